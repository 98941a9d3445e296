"""The sink-token list of the guarded form (include/memvul_hip.h mv_set_sink_tokens), on the GPU.

In the guarded form a sequence that carries a listed token at positions 1 .. len - 2 never runs in the default form: it goes straight into the safe-form
pass, next to the sequences the monitor flags.  Fixtures and engine sizes are the guarded suite's (tests/test_guarded_form_gpu.py: 16 rows, 12 layers; on its
three mixed cases the list [synth.MID_ID] selects exactly the marked reports and anchors — tests/test_sink_routing_cpu.py checks that without a GPU); the list is
[synth.MID_ID] unless a test says otherwise."""
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_guarded_form_gpu as gg  # noqa: E402  (the mixed cases, the ragged batch and the 16-row engines of the guarded suite)
import test_sink_routing_cpu as rc  # noqa: E402  (the matrices of the rule and its numpy restatement)

LOGIT_TOL = gg.LOGIT_TOL
LIST = [synth.MID_ID]
ITEMS = 132  # monitored (head, layer) items per sequence of >= 16 tokens: 12 heads x 11 layers (the pruned last layer feeds none)
BANK = [0, 1, 6, 7]  # two marked anchors and the same two unmarked


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def refs(golden_dir):
    return np.load(os.path.join(golden_dir, "guarded_form_refs.npz")), np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))


def _engine(dims, w, compute, tokens=None):
    eng = gg._engine(dims, w, compute)
    if tokens is not None:
        eng.set_sink_tokens(tokens)
    return eng


# ---- 1. routed equals guarded in bits, but the marked rows run once ------------------------------------------------------------------------------------------------

def _mixed_run(refs, case, tokens):
    """gg._run with the counters of this suite: the 12 anchors one per call, then the 16 reports through forward at S = 256."""
    dims, w, ids, lens, aids, alens, marked, amarked = gg._mixed(refs, case)
    eng = _engine(dims, w, "guarded", tokens)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            aforms, aroutes = [], []
            for g in range(len(alens)):
                eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
                aforms += eng.last_row_forms()
                aroutes.append(eng.route_stats(reset=True))
            a_stats = eng.form_stats(reset=True)
            eng.attention_concentration(reset=True)
            out = eng.forward(ids, lens, want_embed=True)
        return dict(logits=out["logits"], embed=out["embed"], bank=eng.anchor_get(), forms=eng.last_row_forms(), aforms=aforms, aroutes=aroutes, a_stats=a_stats,
                    route=eng.route_stats(), stats=eng.form_stats(), conc=eng.attention_concentration(), sat=eng.x8_saturation(), lens=lens,
                    marked=marked, amarked=amarked)
    finally:
        eng.close()


@pytest.mark.parametrize("case", gg.CASES)
def test_routed_equals_guarded_in_bits_and_the_marked_rows_run_once(gu, refs, case):
    """1. A guarded engine with the list and one without give byte-equal embeddings, bank, logits and row forms on the mixed cases (the monitor flags every marked
    sequence there by a wide margin); the contract holds; only the counters differ: the routed rows are counted by route_stats(), not by form_stats()[1], and
    the monitor never saw them — its item total is 132 x the UNROUTED rows, which is what shows that they ran in no default-form pass."""
    r, p = _mixed_run(refs, case, LIST), _mixed_run(refs, case, None)
    for k in ("embed", "bank", "logits"):
        assert r[k].tobytes() == p[k].tobytes(), k
    assert r["forms"] == p["forms"] and r["aforms"] == p["aforms"]
    err = np.abs(r["logits"] - refs[0][case + "_lg"])
    e = float(err.max())
    forms, aforms = np.array(r["forms"]), np.array(r["aforms"])
    marked, amarked = r["marked"], r["amarked"]
    clean, aclean = np.setdiff1d(np.arange(16), marked), np.setdiff1d(np.arange(12), amarked)
    clean_resc, aclean_resc = int((forms[clean] == "safe").sum()), int((aforms[aclean] == "safe").sum())
    print(f"sink routing {case}: max |logit error| {e:.3e}; routed {r['route']} reports, {sum(r['aroutes'])} anchors; clean reports rescored {clean_resc} of 8, "
          f"clean anchors {aclean_resc} of 6; monitor items with the list {r['conc'][2]}, without {p['conc'][2]}")
    gu.record("sink_routing_mixed", case=case, logits_err=e, err_marked_rows=float(err[marked].max()), err_clean_rows=float(err[clean].max()),
              routed_reports=r["route"], routed_anchors=int(sum(r["aroutes"])), clean_reports_rescored=clean_resc, clean_anchors_rescored=aclean_resc,
              items_total_with_list=r["conc"][2], items_total_without=p["conc"][2])
    assert e <= LOGIT_TOL, e
    assert (forms[marked] == "safe").all() and (aforms[amarked] == "safe").all(), (forms, aforms)
    # the counters: 1 per marked anchor call, 8 after the forward; rescored = the clean rows the monitor flagged, nothing else
    assert r["aroutes"] == [1] * 6 + [0] * 6 and r["route"] == 8
    assert p["aroutes"] == [0] * 12 and p["route"] == 0
    assert r["a_stats"] == (12, aclean_resc) and r["stats"] == (16, clean_resc)
    assert p["a_stats"] == (12, 6 + aclean_resc) and p["stats"] == (16, 8 + clean_resc)
    # the monitor's item total of the forward: the routed rows never ran with it attached
    long_rows = r["lens"] >= 16
    assert p["conc"][2] == ITEMS * int(long_rows.sum())
    assert r["conc"][2] == ITEMS * int(long_rows[clean].sum())
    # a form that routes (or rescores) everything cannot pass
    assert (forms[clean] == "default").sum() >= 4 and (aforms[aclean] == "default").sum() >= 3, (forms, aforms)
    assert r["sat"] == 0


# ---- 2. / 3. / 5. every entry point, the limits of the list, the timing of a list change ----------------------------------------------------------------------------

def _sweep(eng, ids, lens, streams, with_probs):
    eng.set_streams(streams)
    best, idx, ps = eng.bucketed_sweep(ids, lens, 4, with_probs=with_probs)
    order = np.argsort(lens, kind="stable")
    forms = np.empty(len(lens), object)
    forms[order] = eng.corpus_row_forms(0, len(lens))
    out = {"best": best, "best_idx": idx, "forms": forms.tolist()}
    if with_probs:
        out["ps"] = ps
    return out


def _halves(eng, ids, lens):
    t1 = eng.forward_by_length_begin(ids, lens, want_embed=True, min_tokens=1)
    t2 = eng.forward_by_length_begin(ids[::-1].copy(), lens[::-1].copy(), want_embed=True, min_tokens=1)
    assert t1[0] == "pending" and t2[0] == "pending"
    r1 = eng.forward_by_length_end(t1)
    f1 = eng.last_row_forms()
    r2 = eng.forward_by_length_end(t2)
    assert eng.last_row_forms() == f1[::-1]
    assert np.array_equal(r2["embed"], r1["embed"][::-1])
    return {"embed": r1["embed"], "forms": f1}


def _every_entry_point(eng, ids, lens, aids, alens, bank_safe=None, sweeps=((2, False), (2, True), (1, False), (1, True)), full=True):
    """Every entry point once on one engine: {name: {per-row arrays, "forms", "route", "stats", "items"}}; the counters are those of that call alone.  The rows
    are compared through their embeddings (a row's logits depend on the bank, and a guarded bank mixes forms), the resident sweep through the matcher's outputs
    against bank_safe (None: the bank this engine encoded — the safe engine's own)."""
    res = {}

    def call(name, fn):
        eng.route_stats(reset=True)
        eng.form_stats(reset=True)
        eng.attention_concentration(reset=True)
        out = fn()
        if "forms" not in out:
            out["forms"] = eng.last_row_forms()
        out.update(route=eng.route_stats(), stats=eng.form_stats(), items=eng.attention_concentration()[2])
        res[name] = out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng.anchor_reset()

        def bank():
            forms = []
            for a in BANK:
                eng.anchor_append(aids[a:a + 1, :int(alens[a])], alens[a:a + 1])
                forms += eng.last_row_forms()
            return {"embed": eng.anchor_get(), "forms": forms}

        call("anchor_append", bank)
        call("forward", lambda: {"embed": eng.forward(ids, lens, want_embed=True)["embed"]})
        if full:
            call("encode", lambda: {"embed": eng.encode(ids, lens)})
        call("forward_by_length", lambda: {"embed": eng.forward_by_length(ids, lens, want_embed=True, min_tokens=1)["embed"]})
        if full:
            call("begin_end", lambda: _halves(eng, ids, lens))

            def bank_in_one_call():  # four anchors in ONE call, marked and clean interleaved (the clean pair has the marked pair's lengths: either pass has the same shortest row): the bank keeps the caller's order
                rows = [0, 6, 1, 7]
                L = int(alens[rows].max())
                eng.anchor_reset()
                eng.anchor_append(np.ascontiguousarray(aids[rows, :L]), np.ascontiguousarray(alens[rows]))
                return {"embed": eng.anchor_get()}

            call("anchor_append_many", bank_in_one_call)
        eng.anchor_set(res["anchor_append"]["embed"] if bank_safe is None else bank_safe)
        for streams, with_probs in sweeps:
            call(f"sweep_{streams}_{int(with_probs)}", lambda: _sweep(eng, ids, lens, streams, with_probs))
    return res


_shared = {}


def _batch_runs(refs):
    """The ragged batch of the guarded suite through the safe engine, the guarded engine without a list and the guarded engine with it: once per module."""
    if not _shared:
        dims, w, _, _, aids, alens, _, _ = gg._mixed(refs, "mid_all_80_3001")
        ids, lens, marked = gg._ragged_batch(dims.vocab_size)
        assert np.flatnonzero(rc.rule(ids, lens, LIST)).tolist() == marked.tolist()
        _shared.update(dims=dims, w=w, aids=aids, alens=alens, ids=ids, lens=lens, marked=marked)
        for name, compute, tokens in (("safe", "safe", None), ("guarded", "guarded", None), ("routed", "guarded", LIST)):
            eng = _engine(dims, w, compute, tokens)
            try:
                _shared[name] = _every_entry_point(eng, ids, lens, aids, alens, _shared["safe"]["anchor_append"]["embed"] if name != "safe" else None)
            finally:
                eng.close()
    return _shared


def _rows_equal(a, b, rows, keys, what):
    for k in keys:
        for i in rows:
            assert a[k][i].tobytes() == b[k][i].tobytes(), (what, k, int(i))


def _keys(out):
    return [k for k in out if k not in ("forms", "route", "stats", "items")]


def test_every_entry_point_routes_the_marked_rows(gu, refs):
    """2. forward, encode, forward_by_length, its two halves with two tickets in flight, anchor_append (one anchor per call, and four of mixed kinds in one call)
    and bucketed_sweep at 1 and 2 streams with and without P(same): the marked rows are byte-equal to a safe engine's result of the same call, every other row
    to the guarded engine's without the list; route_stats() counts each marked sequence once per call."""
    sh = _batch_runs(refs)
    marked, B = sh["marked"], len(sh["lens"])
    clean = np.setdiff1d(np.arange(B), marked)
    n_long_clean = int((sh["lens"][clean] >= 16).sum())
    for name, out in sh["routed"].items():
        s, g = sh["safe"][name], sh["guarded"][name]
        if name == "anchor_append":
            m, c, n = [0, 1], [2, 3], 4
        elif name == "anchor_append_many":
            m, c, n = [0, 2], [1, 3], 4
        else:
            m, c, n = marked, clean, B
        _rows_equal(out, s, m, _keys(out), name + " marked")
        _rows_equal(out, g, c, _keys(out), name + " clean")
        calls = 2 if name == "begin_end" else 1
        assert out["route"] == calls * len(m) and g["route"] == 0 and s["route"] == 0, (name, out["route"])
        if name != "anchor_append_many":
            forms = np.array(out["forms"])
            assert (forms[m] == "safe").all() and forms.tolist() == g["forms"], (name, forms)
            resc = int((forms[c] == "safe").sum())
            assert out["stats"] == (calls * n, calls * resc) and g["stats"] == (calls * n, calls * (len(m) + resc)), (name, out["stats"], g["stats"])
            gu.record("sink_routing_entry_point", entry=name, routed=out["route"], clean_rows_rescored=resc, rows=n)
        if n == B:  # the routed rows fed no monitor item (every row of this batch has >= 16 tokens)
            assert g["items"] == calls * ITEMS * B and out["items"] == calls * ITEMS * n_long_clean, (name, out["items"], g["items"])


def test_the_limits_of_the_list(gu, refs):
    """3. An empty list is the guarded form, byte for byte, counters included; a list naming a token every row carries is the safe form and nothing runs in
    the default form; on a safe and on a precise engine the list changes nothing."""
    sh = _batch_runs(refs)
    dims, w, aids, alens, ids, lens = (sh[k] for k in ("dims", "w", "aids", "alens", "ids", "lens"))
    B = len(lens)
    bank_safe = sh["safe"]["anchor_append"]["embed"]
    # empty (set, then cleared)
    eng = _engine(dims, w, "guarded", LIST)
    try:
        eng.set_sink_tokens([])
        assert eng.sink_tokens() == []
        got = _every_entry_point(eng, ids, lens, aids, alens, bank_safe)
    finally:
        eng.close()
    for name, out in got.items():
        g = sh["guarded"][name]
        _rows_equal(out, g, range(len(out["embed"] if "embed" in out else out["best"])), _keys(out), name + " empty list")
        assert out["route"] == 0 and out["stats"] == g["stats"] and out["items"] == g["items"] and out["forms"] == g["forms"], name
    # a token in every row (position 1 of every report and anchor: all of them are longer than 2 tokens)
    EVERY = 1999
    ids2, aids2 = ids.copy(), aids.copy()
    ids2[:, 1] = EVERY
    aids2[:, 1] = EVERY
    assert rc.rule(ids2, lens, [EVERY]).all() and rc.rule(aids2, alens, [EVERY]).all()
    outs = {}
    for name, compute, tokens in (("safe", "safe", None), ("all", "guarded", [EVERY])):
        eng = _engine(dims, w, compute, tokens)
        try:
            outs[name] = _every_entry_point(eng, ids2, lens, aids2, alens, outs["safe"]["anchor_append"]["embed"] if name != "safe" else None,
                                            sweeps=((2, True), (1, False)), full=False)
        finally:
            eng.close()
    for name, out in outs["all"].items():
        s = outs["safe"][name]
        n = len(out["embed"] if "embed" in out else out["best"])
        _rows_equal(out, s, range(n), _keys(out), name + " every row listed")
        assert out["items"] == 0 and out["stats"] == (n, 0) and out["route"] == n and set(out["forms"]) == {"safe"}, (name, out["items"], out["stats"], out["route"])
    # kept, not acted on, outside the guarded form
    for compute in ("safe", "precise"):
        res = {}
        for tokens in (None, LIST):
            eng = _engine(dims, w, compute, tokens)
            try:
                assert eng.sink_tokens() == (tokens or [])
                res[bool(tokens)] = _every_entry_point(eng, ids, lens, aids, alens, bank_safe, sweeps=((2, True),), full=False)
            finally:
                eng.close()
        for name, out in res[True].items():
            n = len(out["embed"] if "embed" in out else out["best"])
            _rows_equal(out, res[False][name], range(n), _keys(out), f"{name} {compute}")
            assert out["route"] == 0 and out["forms"] == res[False][name]["forms"] and out["items"] == res[False][name]["items"], (compute, name)


def test_a_list_change_does_not_reach_work_already_made(gu, refs):
    """5. A ticket begun before set_sink_tokens([]) comes back with its marked rows routed; a sweep run before a list change keeps its routing at
    corpus_results — and the other way round: what was begun without the list is not routed by a list set later."""
    sh = _batch_runs(refs)
    dims, w, aids, alens, ids, lens, marked = (sh[k] for k in ("dims", "w", "aids", "alens", "ids", "lens", "marked"))
    B = len(lens)
    order = np.argsort(lens, kind="stable")
    eng = _engine(dims, w, "guarded", LIST)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            eng.anchor_set(sh["safe"]["anchor_append"]["embed"])

            def sweep_with_change(before, after):
                eng.set_sink_tokens(before)
                eng.route_stats(reset=True)
                eng.form_stats(reset=True)
                eng.corpus_upload(ids[order], lens[order])
                sl = lens[order]
                for s0 in range(0, B, 4):
                    eng.corpus_run(s0, 4, 4, keep_probs=True, s_eff=int(sl[s0 + 3]))
                eng.set_sink_tokens(after)
                best, idx, ps = eng.corpus_results(0, B, with_probs=True)
                inv = np.empty(B, np.int64)
                inv[order] = np.arange(B)
                return {"best": best[inv], "best_idx": idx[inv], "ps": ps[inv]}, eng.route_stats(), eng.form_stats()

            def ticket_with_change(before, after):
                eng.set_sink_tokens(before)
                eng.route_stats(reset=True)
                eng.form_stats(reset=True)
                t = eng.forward_by_length_begin(ids, lens, want_embed=True, min_tokens=1)
                assert t[0] == "pending"
                eng.set_sink_tokens(after)
                out = eng.forward_by_length_end(t)
                return {"embed": out["embed"]}, eng.last_row_forms(), eng.route_stats(), eng.form_stats()

            want = sh["routed"]["sweep_2_1"]
            got, route, stats = sweep_with_change(LIST, [])
            _rows_equal(got, want, range(B), ("best", "best_idx", "ps"), "sweep, list cleared before the results")
            assert route == len(marked) and stats == want["stats"]
            want = sh["guarded"]["sweep_2_1"]
            got, route, stats = sweep_with_change([], LIST)
            _rows_equal(got, want, range(B), ("best", "best_idx", "ps"), "sweep, list set before the results")
            assert route == 0 and stats == want["stats"]

            eng.anchor_reset()
            for a in BANK:
                eng.anchor_append(aids[a:a + 1, :int(alens[a])], alens[a:a + 1])
            want = sh["routed"]["forward_by_length"]
            got, forms, route, stats = ticket_with_change(LIST, [])
            _rows_equal(got, want, range(B), ("embed",), "ticket, list cleared before the end")
            assert (np.array(forms)[marked] == "safe").all() and forms == want["forms"] and route == len(marked) and stats == want["stats"]
            want = sh["guarded"]["forward_by_length"]
            got, forms, route, stats = ticket_with_change([], LIST)
            _rows_equal(got, want, range(B), ("embed",), "ticket, list set before the end")
            assert forms == want["forms"] and route == 0 and stats == want["stats"]
    finally:
        eng.close()


# ---- 4. the kernel -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_kernel_flags_what_the_rule_flags(gu):
    """4. corpus_route_flags after corpus_upload of the CPU test's matrices (both widths, the 70 rows, every placement and list) equals route_scan and numpy —
    again after set_sink_tokens with another list and no new upload, and again after a new upload; and at row pitches that are no multiple of four ints (the
    kernel's 16-byte chunks are aligned in the array, not in the row)."""
    from memvul_amd.binding import Engine

    engines = {}
    n = 0
    try:
        for vocab in (2048, 30522):
            dims, w = gu.weights_for(dict(layers=2, vocab_size=vocab), {})
            eng = Engine(0, vocab_size=vocab, layers=2, max_tokens=4096, max_batch=16, max_anchors=16)
            engines[vocab] = eng
            eng.load_state_dict(w, "guarded")
        prev = {}
        for S, vocab, name, tokens, ids, lens in rc.cases():
            eng = engines[vocab]
            if vocab in prev:  # the corpus of the case before, under this case's list: no new upload
                p_ids, p_lens = prev[vocab]
                eng.set_sink_tokens(tokens)
                assert np.array_equal(eng.corpus_route_flags(0, rc.B), rc.rule(p_ids, p_lens, tokens)), (S, vocab, name, "list changed")
            eng.set_sink_tokens(tokens)
            eng.corpus_upload(ids, lens)  # a new upload under a list already set
            want = rc.rule(ids, lens, tokens)
            got = eng.corpus_route_flags(0, rc.B)
            assert np.array_equal(got, want), (S, vocab, name, np.flatnonzero(got != want))
            assert np.array_equal(got, Engine.route_scan(ids, lens, tokens, vocab_size=vocab))
            assert np.array_equal(eng.corpus_route_flags(17, 30), want[17:47])
            prev[vocab] = (ids, lens)
            n += 1
            if name == "many":  # odd pitches: rows that start at every offset of a 16-byte chunk, an array that ends inside one
                for S2 in (61, 63):
                    ids2 = np.ascontiguousarray(ids[:, :S2])
                    lens2 = np.minimum(lens, S2).astype(np.int32)
                    ids2[:, S2 - 1] = tokens[3]
                    eng.corpus_upload(ids2, lens2)
                    assert np.array_equal(eng.corpus_route_flags(0, rc.B), rc.rule(ids2, lens2, tokens)), (S, vocab, S2)
                prev.pop(vocab)
        assert n == 20
        eng = engines[2048]
        eng.set_sink_tokens([])
        assert not eng.corpus_route_flags(0, rc.B).any()
        gu.record("sink_routing_kernel", matrices=n, rows=rc.B)
    finally:
        for eng in engines.values():
            eng.close()


# ---- 6. strictness -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_list_is_checked_strictly(gu, monkeypatch):
    from memvul_amd.binding import Engine

    dims, w = gu.weights_for(gg.L2, gg.WK)
    kw = dict(vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=4096, max_batch=16, max_anchors=16)
    monkeypatch.delenv("MEMVUL_SINK_TOKENS", raising=False)
    monkeypatch.delenv("MEMVUL_FORM", raising=False)
    eng = Engine(0, **kw)
    try:
        with pytest.raises(RuntimeError, match=r"\(-3\).*finalize"):  # MV_ERR_STATE
            eng.set_sink_tokens([5])
        eng.load_state_dict(w, "guarded")
        assert eng.sink_tokens() == [] and eng.route_stats() == 0
        with pytest.raises(RuntimeError, match=r"mv_corpus_route_flags failed \(-3\)"):
            eng.corpus_route_flags(0, 1)
        eng.set_sink_tokens([7, 7, 9])
        assert eng.sink_tokens() == [7, 7, 9]
        for bad in ([dims.vocab_size], [-1], [3, dims.vocab_size], list(range(65))):
            with pytest.raises(RuntimeError, match=r"mv_set_sink_tokens failed \(-1\)"):  # MV_ERR_INVALID, the list unchanged
                eng.set_sink_tokens(bad)
            assert eng.sink_tokens() == [7, 7, 9]
        eng.set_sink_tokens(list(range(64)))
        assert eng.sink_tokens() == list(range(64))
        eng.set_sink_tokens([])
        assert eng.sink_tokens() == []
    finally:
        eng.close()
    for compute in ("f16", "f32"):
        eng = Engine(0, **kw)
        try:
            eng.load_state_dict(w, compute)
            with pytest.raises(RuntimeError, match=r"\(-3\).*MV_F16"):
                eng.set_sink_tokens([5])
        finally:
            eng.close()
    monkeypatch.setenv("MEMVUL_SINK_TOKENS", "1012")
    monkeypatch.setenv("MEMVUL_FORM", "default")
    eng = Engine(0, **kw)
    try:
        with pytest.raises(ValueError, match="guarded form only"):
            eng.load_state_dict(w, "precise")
    finally:
        eng.close()
    monkeypatch.setenv("MEMVUL_FORM", "guarded")
    eng = Engine(0, **kw)
    try:
        eng.load_state_dict(w, "precise")
        assert eng.form == "guarded" and eng.sink_tokens() == [1012]
    finally:
        eng.close()
    monkeypatch.delenv("MEMVUL_FORM")
    eng = Engine(0, sink_tokens=[3, 4], **kw)  # engine_options["sink_tokens"] of ModelMemory / ModelSingle arrives here; it wins over the environment
    try:
        eng.load_state_dict(w, "guarded")
        assert eng.sink_tokens() == [3, 4]
    finally:
        eng.close()


# ---- 7. nothing listed, nothing changed -------------------------------------------------------------------------------------------------------------------------------

def test_nothing_listed_nothing_changed(gu):
    """7. The random-init 12-layer family with a list whose token occurs in no row: forward, forward_by_length and bucketed_sweep are byte-equal to the default
    form's, nothing is routed, nothing is rescored."""
    dk, wk = dict(layers=12), dict()
    dims, w = gu.weights_for(dk, wk)
    kw = dict(max_tokens=32 * 256, max_batch=32, max_anchors=16)
    ids, lens = synth.make_ids(32, 256, dims.vocab_size, seed=synth.SEED + 5, ragged=True, min_len=20)
    aids, alens = synth.make_ids(8, 64, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=16)
    ABSENT = [5, 6]
    assert not np.isin(ids, ABSENT).any() and not np.isin(aids, ABSENT).any()

    def run(eng):
        eng.anchor_reset()
        eng.form_stats(reset=True)
        eng.anchor_append(aids, alens)
        out = {"bank": eng.anchor_get()}
        for k, v in eng.forward(ids, lens, want_embed=True).items():
            out["forward_" + k] = v
        for k, v in eng.forward_by_length(ids, lens, want_embed=True, min_tokens=1).items():
            out["by_length_" + k] = v
        out["sweep_best"], out["sweep_idx"], out["sweep_ps"] = eng.bucketed_sweep(ids, lens, 8, with_probs=True)
        eng.anchor_reset()
        return out

    od = run(gu.engine_for(dk, wk, compute_dtype="precise", **kw))
    g = gu.engine_for(dk, wk, compute_dtype="guarded", **kw)
    try:
        g.set_sink_tokens(ABSENT)
        g.route_stats(reset=True)
        og = run(g)
        for k in od:
            assert og[k].tobytes() == od[k].tobytes(), k
        assert g.route_stats() == 0 and g.form_stats() == (8 + 3 * 32, 0)
        assert not g.corpus_route_flags(0, 32).any() and set(g.corpus_row_forms(0, 32)) == {"default"}
    finally:
        g.set_sink_tokens([])  # (the engine is shared with the guarded suite)
