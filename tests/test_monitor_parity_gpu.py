"""The attention kernel's concentration monitor (memvul_amd/csrc/attention_v2.h, AttnArgs::conc / AttnArgs::seq_over) against a float64 reference, on the GPU.

The monitor's number — the collision mass of the [CLS] row on the ordinary keys, per (layer, sequence, head) item — chooses the safe form (the sink warning,
MEMVUL_ON_SINK=safe), decides per sequence what the guarded form encodes again (engine.hip guard_flagged) and is reported by memvul_amd.audit.  Reference:
oracle/concentration.py on the exact float64 forward, committed as tests/golden/monitor_refs.npz by scripts/make_monitor_refs.py (its docstring describes the
models, the lengths and the moving sink position).  Observability without an ABI change: one sequence per call after attention_concentration(reset=True) gives
that sequence's (max_collision, items_over, items_total).

The band.  delta_abs = 3 x the largest |rounding model - exact| over every monitored item of the fixture (shipped default and safe form; the model only sizes the
margin, no GPU value enters it) = 3 x 1.401e-3 = 4.204e-3 (stored in the fixture); an item's band is delta_abs + 2^-10 x its collision mass (the model reads P unrounded, the kernel squares
fp16 probabilities).  A count must lie in [#(exact > 0.25 + band), #(exact > 0.25 - band)], a maximum within the band of the exact maximum, items_total is exact.

At padded widths 192 and 384 the default form's GEMMs take their form from the WHOLE pass (engine.hip encode_dev: the [CLS]-row form when the pass's shortest
sequence has 128 tokens, else both terms in every row), so a row's bits there depend on the shortest row it travels with: where a single row is compared BIT FOR
BIT with its batch, it is given a 15-token companion — a sequence the monitor does not look at — whenever the batch's shortest row is below 128 tokens.

Every test records what it measured (gu.record "monitor_*": the largest |GPU - exact| per width and form, the rows at the rule's edge); DESIGN.md section 2 and
profiles/LEDGER.md say what has been measured so far."""
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_monitor_refs as mk  # noqa: E402
from oracle import concentration as conc  # noqa: E402

COMPUTE = {"default": "precise", "safe": "safe"}  # form -> compute dtype name
T = conc.THRESHOLD
CLS_MIN_LEN = 128  # engine.hip mv_handle::cls_min_len (MEMVUL_CLS_ASIDE_MIN_LEN's default)
BIG = dict(max_tokens=16384, max_batch=128, max_anchors=128)


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def refs(golden_dir):
    r = np.load(os.path.join(golden_dir, "monitor_refs.npz"))
    return {k: r[k] for k in r.files}


class _Sink(dict):
    """The `sink` argument of synth.make_weights in a form gpu_util's caches can key on."""

    def __hash__(self):
        return hash(tuple(sorted(self.items())))


def _w_kw(refs, model):
    token, rows, _, seed, _ = mk.MODELS[model]
    return dict(mk.KW, seed=seed, sink=_Sink(token=token, rows=rows, gains=tuple(float(g) for g in refs[model + "_gains"])))


def _engine(gu, refs, model, compute, prune=True, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gu.engine_for(mk.DIMS, _w_kw(refs, model), compute_dtype=compute, env=None if prune else {"MEMVUL_CLS_PRUNE": "0"}, **kw)


def _quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the default form warns once about the sink it sees: tests/test_gpu_parity.py)
        return f(*a, **k)


_COMPANION = {}


def _companion(W):
    """A 15-token sequence at width W: the monitor does not look at it, and a pass that holds it runs in the both-terms form at 192 / 384."""
    if W not in _COMPANION:
        ids, _ = synth.make_ids(1, W, mk.DIMS["vocab_size"], seed=77)
        ids[0, 14], ids[0, 15:] = synth.SEP_ID, 0
        _COMPANION[W] = ids
    return _COMPANION[W]


def _read_row(eng, ids_row, n, W, ragged_pass=False):
    """(max_collision, items_over, items_total) of ONE sequence encoded at width W.  ragged_pass: in the pass form of a batch whose shortest row is below
    CLS_MIN_LEN tokens (the module docstring)."""
    ids, lens = ids_row[None, :W], np.array([n], np.int32)
    if ragged_pass and mk.padded(W) in (192, 384):
        ids, lens = np.concatenate([ids, _companion(W)]), np.array([n, 15], np.int32)
    eng.attention_concentration(reset=True)
    _quiet(eng.encode, np.ascontiguousarray(ids, np.int32), lens)
    return eng.attention_concentration()


def _interval(e, n, delta_abs):
    """Of one sequence's exact items e [layers, heads]: (fewest, most) items over the threshold the band allows, the exact maximum and its band."""
    if n < conc.MIN_LEN:
        return 0, 0, 0.0, 0.0
    b = mk.band(e, delta_abs)
    return int((e > T + b).sum()), int((e > T - b).sum()), float(e.max()), float(mk.band(e.max(), delta_abs))


def _check_row(got, e, n, layers, delta_abs, what, bad):
    """One sequence's reading against its exact items; failures are collected (every figure of a run is seen), returns |GPU max - exact max|."""
    m, over, total = got
    lo, hi, top, b = _interval(e, n, delta_abs)
    if total != (12 * layers if n >= conc.MIN_LEN else 0):
        bad.append(f"{what}: items_total {total}, want {12 * layers if n >= conc.MIN_LEN else 0}")
    if not lo <= over <= hi:
        bad.append(f"{what}: items_over {over} outside [{lo}, {hi}] (exact count {int((e > T).sum()) if n >= conc.MIN_LEN else 0})")
    if not abs(m - top) <= b:
        bad.append(f"{what}: max_collision {m:.6f}, exact {top:.6f}, band {b:.2e}")
    return abs(m - top)


# ---- a. per sequence, at every width, in both forms, pruned and not ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("form", ["default", "safe"])
@pytest.mark.parametrize("model", list(mk.MODELS))
def test_every_sequence_reads_its_float64_collision_mass(gu, refs, model, form, prune):
    """a. 48 sequences per model (6 widths x 8 lengths, the sink token at position 1, len - 2, len // 2, inside every 128-key chunk, nowhere), one per call:
    items_total exactly 12 x the monitored layers from 16 tokens on and 0 below, items_over inside the interval the band allows, max_collision within the band
    of the exact maximum."""
    eng = _engine(gu, refs, model, COMPUTE[form], prune)
    assert eng.form == form
    layers = mk.DIMS["layers"] - (1 if prune else 0)
    delta_abs = float(refs["delta_abs"])
    bad, gap, edge = [], {}, 0
    for W in mk.WIDTHS:
        ids, lens, pos, names = mk.case_inputs(model, W)
        ex = refs["%s_%d_exact" % (model, W)][:layers]
        gap[W] = 0.0
        for b, n in enumerate(lens):
            n = int(n)
            what = f"{model}, {form} form, {'pruned' if prune else 'MEMVUL_CLS_PRUNE=0'}, width {W}, len {n}, sink {names[b]} at {pos[b]}"
            got = _read_row(eng, ids[b], n, W)
            gap[W] = max(gap[W], _check_row(got, ex[:, b], n, layers, delta_abs, what, bad))
            lo, hi = _interval(ex[:, b], n, delta_abs)[:2]
            edge += lo != hi
    print(f"{model} {form} prune={prune}: largest |GPU max - exact max| per width {gap}; rows with a band item {edge} of 48")
    gu.record("monitor_rows", model=model, form=form, prune=prune, delta_abs=delta_abs, rows_with_band_items=int(edge), **{"gap_%d" % W: g for W, g in gap.items()})
    assert not bad, "\n".join(bad)


# ---- b. the excluded keys ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["default", "safe"])
def test_the_excluded_keys_are_cls_and_sep_and_no_ordinary_token(gu, refs, form):
    """b. 80 % of the mass on [SEP] or on [CLS]: what is left on the ordinary keys is small, and the monitor reads that small number (no item over, the maximum
    within the band of an exact maximum below 0.2, where 0.8^2 = 0.64 would be read if the sink key were counted).  The sink on the FIRST ordinary token (position 1 — the engine keeps [SEP] in row 1, the token itself in row
    len - 1) and on the LAST (len - 2) is counted in full: the exact maximum is above 0.4 there, and the monitor reads it within the band."""
    delta_abs, bad, seen = float(refs["delta_abs"]), [], {}
    for model in ("sep_cls_80", "cls_all_80", "mid_cls_52", "mid_all_50"):
        eng = _engine(gu, refs, model, COMPUTE[form])
        control = model in ("sep_cls_80", "cls_all_80")
        for W in mk.WIDTHS:
            ids, lens, pos, names = mk.case_inputs(model, W)
            ex = refs["%s_%d_exact" % (model, W)][:2]
            for b, n in enumerate(lens):
                n = int(n)
                top = float(ex[:, b].max())
                if n < 64 or (not control and (names[b] not in ("first", "last") or top <= 0.4)):
                    continue
                what = f"{model}, {form} form, width {W}, len {n}, sink {names[b]} at {pos[b]}"
                m, over, total = _read_row(eng, ids[b], n, W)
                key = "control" if control else names[b]
                seen[key] = seen.get(key, 0) + 1
                if control:
                    assert top < 0.2, (what, top)  # (the fixture's own condition: tests/test_monitor_parity_cpu.py)
                    if over != 0:
                        bad.append(f"{what}: {over} items over, exact maximum {top:.4f}")
                elif not m > T:
                    bad.append(f"{what}: max_collision {m:.4f} not over the threshold, exact {top:.4f}")
                if abs(m - top) > mk.band(top, delta_abs) or total != 24:
                    bad.append(f"{what}: max_collision {m:.6f}, exact {top:.6f}, items_total {total}")
    print(f"excluded keys, {form} form: rows looked at {seen}")
    gu.record("monitor_excluded_keys", form=form, **seen)
    assert seen.get("control", 0) >= 40 and seen.get("first", 0) >= 4 and seen.get("last", 0) >= 4, seen
    assert not bad, "\n".join(bad)


# ---- c. whole batches: attribution, and every entry point ----------------------------------------------------------------------------------------------------

_singles = {}


def _batch_singles(gu, refs, B, S):
    """The (max, over, total) of every row of batch (B, S) alone at width S in the batch's pass form, and alone at the padded length of its own token count."""
    if (B, S) not in _singles:
        eng = _engine(gu, refs, mk.BATCH_MODEL, "precise", **BIG)
        ids, lens, _ = mk.batch_inputs(B, S)
        at_s = [_read_row(eng, ids[i], int(lens[i]), S, ragged_pass=True) for i in range(B)]
        own = [_read_row(eng, ids[i], int(lens[i]), min(S, mk.padded(int(lens[i])))) for i in range(B)]
        _singles[(B, S)] = (at_s, own)
    return _singles[(B, S)]


def _sums(rows):
    return (max(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows))


def _sweep_batch(lens, S):
    """Rows per pass of a resident sweep such that, at 192 / 384, every pass has the batch's pass form (a row below CLS_MIN_LEN tokens in it)."""
    B = len(lens)
    for nb in (8, 12, 16, 24, B):
        if mk.padded(S) not in (192, 384) or all(int(lens[s:s + nb].min()) < CLS_MIN_LEN for s in range(0, B, nb)):
            return nb


@pytest.mark.parametrize("B,S", mk.BATCHES)
def test_a_batch_counts_what_its_rows_count_alone(gu, refs, B, S):
    """c. tests/test_gpu_kernels.py test_attention_persistent_item_loop's batches (more units than resident workgroups, uneven tails, one to four key chunks),
    ragged, every other row marked with the sink token at a moving position, rows 2 and 3 of 15 and 16 tokens.  Every row alone is inside the band of its exact
    items; through encode, anchor_append, forward and the resident sweep on one stream and on two the batch's items_over / items_total are the SUMS of its rows'
    and its max_collision the largest of theirs bit for bit; forward_by_length the same against the rows alone at the padded length of their own token count."""
    delta_abs = float(refs["delta_abs"])
    ids, lens, pos = mk.batch_inputs(B, S)
    ex = refs["batch_%d_%d_exact" % (B, S)][:2]
    at_s, own = _batch_singles(gu, refs, B, S)
    bad, gap = [], 0.0
    for i in range(B):
        for name, rows in (("width %d" % S, at_s), ("its own width", own)):
            gap = max(gap, _check_row(rows[i], ex[:, i], int(lens[i]), 2, delta_abs, f"batch ({B}, {S}) row {i} alone at {name}, len {int(lens[i])}, sink at {pos[i]}", bad))
    assert not bad, "\n".join(bad)
    lo = sum(_interval(ex[:, i], int(lens[i]), delta_abs)[0] for i in range(B))
    hi = sum(_interval(ex[:, i], int(lens[i]), delta_abs)[1] for i in range(B))
    top = float((ex * (lens >= conc.MIN_LEN)[None, :, None]).max())
    eng = _engine(gu, refs, mk.BATCH_MODEL, "precise", **BIG)
    assert eng.form == "default"
    seen = {}

    def through(name, call, want):
        eng.attention_concentration(reset=True)
        _quiet(call)
        got = seen[name] = eng.attention_concentration()
        assert got[2] == 24 * int((lens >= conc.MIN_LEN).sum()), (name, got)
        assert lo <= got[1] <= hi and abs(got[0] - top) <= mk.band(top, delta_abs), (name, got, (lo, hi), top)
        assert got[1:] == want[1:], (name, got, want)
        assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes(), (name, got, want)

    try:
        eng.anchor_reset()
        through("encode", lambda: eng.encode(ids, lens), _sums(at_s))
        through("anchor_append", lambda: eng.anchor_append(ids, lens), _sums(at_s))
        assert eng.n_anchors == B
        through("forward", lambda: eng.forward(ids, lens), _sums(at_s))
        through("forward_by_length", lambda: eng.forward_by_length(ids, lens, min_tokens=1), _sums(own))
        nb = _sweep_batch(lens, S)
        eng.corpus_upload(ids, lens)
        for streams in (1, 2):
            eng.set_streams(streams)
            through("corpus_run, %d stream(s), %d rows per pass" % (streams, nb), lambda: (eng.corpus_run(0, B, nb), eng.corpus_results(0, B)), _sums(at_s))
    finally:
        eng.set_streams(2)
        eng.anchor_reset()
    print(f"batch ({B}, {S}): {seen}; exact count in [{lo}, {hi}], exact maximum {top:.6f}")
    gu.record("monitor_batches", B=B, S=S, gap_rows_alone=gap, items_over=seen["encode"][1], items_total=seen["encode"][2], max_collision=seen["encode"][0],
              exact_interval=[lo, hi], exact_max=top, items_over_by_length=seen["forward_by_length"][1])


# ---- d. the guarded form, row by row -------------------------------------------------------------------------------------------------------------------------

def _clear_verdicts(ex, lens, delta_abs, layers):
    """(verdict of the rule on the exact count, True where no band item can change it)."""
    _, _, v_lo, v_hi = mk.verdicts(ex, lens, delta_abs, layers)
    return v_lo, v_lo == v_hi


@pytest.mark.parametrize("B,S", mk.BATCHES)
def test_the_guarded_form_rescores_exactly_the_rows_the_rule_names(gu, refs, B, S):
    """d. On the batches of c: last_row_forms()[i] is "safe" exactly when the host rule holds on the GPU's OWN count of row i (the row alone on a default-form
    engine), and equals the rule on the exact count wherever no band item can change that; form_stats() and the resident sweep's corpus_row_forms agree; rows
    of fewer than 16 tokens stay in the default form."""
    delta_abs = float(refs["delta_abs"])
    ids, lens, pos = mk.batch_inputs(B, S)
    at_s, own = _batch_singles(gu, refs, B, S)
    ex = refs["batch_%d_%d_exact" % (B, S)]
    v_exact, clear = _clear_verdicts(ex, lens, delta_abs, 2)
    g = _engine(gu, refs, mk.BATCH_MODEL, "guarded", **BIG)
    assert g.form == "guarded"
    try:
        g.anchor_reset()
        g.anchor_set(np.zeros((2, 512), np.float32))
        for name, call, rows in (("encode", lambda: g.encode(ids, lens), at_s), ("forward", lambda: g.forward(ids, lens), at_s),
                                 ("forward_by_length", lambda: g.forward_by_length(ids, lens, min_tokens=1), own)):
            want = conc.rule([r[1] for r in rows], lens, 2)
            g.form_stats(reset=True)
            _quiet(call)
            forms = np.array(g.last_row_forms()) == "safe"
            wrong = np.flatnonzero(forms != want)
            assert not len(wrong), (name, [(int(i), int(lens[i]), int(pos[i]), rows[i]) for i in wrong])
            assert (forms[clear] == v_exact[clear]).all(), (name, np.flatnonzero(clear & (forms != v_exact)))
            assert not forms[lens < conc.MIN_LEN].any() and g.form_stats() == (B, int(forms.sum())), (name, g.form_stats())
            if name == "encode":
                first = forms
        nb = _sweep_batch(lens, S)
        g.corpus_upload(ids, lens)
        for streams in (1, 2):
            g.set_streams(streams)
            g.form_stats(reset=True)
            _quiet(lambda: (g.corpus_run(0, B, nb), g.corpus_results(0, B)))
            swept = np.array(g.corpus_row_forms(0, B)) == "safe"
            assert np.array_equal(swept, first), (streams, np.flatnonzero(swept != first))
            assert g.form_stats() == (B, int(first.sum()))
    finally:
        g.set_streams(2)
        g.anchor_reset()
    n_edge = int((~clear).sum())
    print(f"guarded form, batch ({B}, {S}): {int(first.sum())} of {B} rows rescored ({int(v_exact.sum())} by the exact count); {n_edge} rows at the rule's edge")
    gu.record("monitor_guarded_batches", B=B, S=S, rescored=int(first.sum()), rescored_by_exact_count=int(v_exact.sum()), rows_at_the_rules_edge=n_edge)
    assert first[0::2][lens[0::2] >= 64].mean() > 0.5 and not first[1::2][lens[1::2] >= 64].mean() > 0.5  # (the marked rows mostly are, the unmarked mostly not)


@pytest.mark.parametrize("case", mk.GUARDED_CASES)
def test_the_guarded_fixture_cases_row_by_row(gu, refs, case):
    """d. The three mixed batches of tests/golden/guarded_form_refs.npz (12 layers, 132 items per sequence, rescored at >= 3; their clean rows read 0 - 3 by the
    exact forward, the rule's edge): 16 reports through forward at 256 tokens, 12 anchors appended one per call — the form of every row is the rule on the GPU's
    own count of that row, and the rule on the exact count wherever no band item can change it."""
    from memvul_amd.binding import Engine

    delta_abs = float(refs["delta_abs"])
    dims, w, ids, lens, aids, alens, _, _ = mk.guarded_inputs(case)
    all_lens = np.concatenate([lens, alens])
    ex = refs["guarded_%s_exact" % case]
    v_exact, clear = _clear_verdicts(ex, all_lens, delta_abs, 11)
    rows = [(ids[i], int(lens[i]), 256) for i in range(16)] + [(aids[g], int(alens[g]), int(alens[g])) for g in range(12)]
    counts, forms, bad = [], [], []
    engs = {c: Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=16 * 512, max_batch=16, max_anchors=16) for c in ("precise", "guarded")}
    try:
        for c, eng in engs.items():
            _quiet(eng.load_state_dict, w, c)
        for i, (row, n, W) in enumerate(rows):
            got = _read_row(engs["precise"], row, n, W)
            counts.append(got[1])
            _check_row(got, ex[:, i], n, 11, delta_abs, f"{case} {'report' if i < 16 else 'anchor'} {i % 16 if i < 16 else i - 16}, len {n}", bad)
        g = engs["guarded"]
        g.form_stats(reset=True)
        aforms = []
        for a in range(12):
            _quiet(g.anchor_append, aids[a:a + 1, :int(alens[a])], alens[a:a + 1])
            aforms += g.last_row_forms()
        _quiet(g.forward, ids, lens)
        forms = np.array(g.last_row_forms() + aforms) == "safe"
        stats = g.form_stats()
    finally:
        for eng in engs.values():
            eng.close()
    assert not bad, "\n".join(bad)
    want = conc.rule(counts, all_lens, 11)
    n_edge = int((~clear).sum())
    print(f"{case}: GPU counts {counts}; rescored {int(forms.sum())} of 28; rows at the rule's edge {n_edge}")
    gu.record("monitor_guarded_fixture", case=case, counts=[int(c) for c in counts], rescored=int(forms.sum()), rows_at_the_rules_edge=n_edge)
    assert np.array_equal(forms, want), (np.flatnonzero(forms != want), counts)
    assert (forms[clear] == v_exact[clear]).all(), np.flatnonzero(clear & (forms != v_exact))
    assert stats == (28, int(forms.sum()))


# ---- e. the other compute dtypes -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compute", ["f16", "f32"])
def test_the_other_compute_dtypes_keep_no_monitor(gu, refs, compute):
    """e. MV_F16 and MV_F32 read (0.0, 0, 0) after the calls that fill the counters of MV_F16X8."""
    eng = _engine(gu, refs, "mid_cls_52", compute)
    ids, lens, _, _ = mk.case_inputs("mid_cls_52", 256)
    eng.attention_concentration(reset=True)
    try:
        eng.anchor_reset()
        eng.encode(ids, lens)
        eng.anchor_append(ids[:2], lens[:2])
        eng.forward(ids, lens)
        eng.forward_by_length(ids, lens, min_tokens=1)
        eng.bucketed_sweep(ids, lens, 4)
        assert eng.attention_concentration() == (0.0, 0, 0)
        assert eng.form == "default" and set(eng.last_row_forms()) == {"default"}
    finally:
        eng.anchor_reset()
    # ... and the same calls do fill them on the default compute dtype
    p = _engine(gu, refs, "mid_cls_52", "precise")
    p.attention_concentration(reset=True)
    _quiet(p.encode, ids, lens)
    assert p.attention_concentration()[2] == 24 * int((lens >= conc.MIN_LEN).sum())
