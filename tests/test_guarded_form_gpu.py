"""The GUARDED form of compute dtype MV_F16X8 (include/memvul_hip.h MV_FORM_GUARDED; binding compute dtype name "guarded"), on the GPU.

Every sequence runs in the default form with the concentration monitor also counting per sequence; a sequence with more than 2 % of its own monitored (head,
layer) items over a collision mass of 0.25 is encoded again in the safe form, at the width of the pass it first ran in, and only its results are replaced.  The
fixture (scripts/make_guarded_form_refs.py) mixes, per sink case, the case's 8 issue reports and 6 anchors with the same sequences without the sink token.

What the exact CPU forward counts on the three fixture cases (items over 0.25 of the 132 monitored per sequence; rescored at >= 3):
    case              marked reports   clean reports       marked anchors   clean anchors
    mid_all_80_3001   125 - 127        0,0,0,0,1,0,0,0     104 - 132        2,0,1,0,1,0
    mid_all_50_3002   35 - 106         0,0,0,0,1,1,0,0     28 - 79          0,0,0,1,0,0
    mid_cls_80_3003   119 - 124        1,3,2,3,1,0,1,1     64 - 132         0,1,2,0,0,8
Every marked sequence is flagged with a wide margin; a few clean ones sit at the rule's edge (rescoring those is a cost, not an error, and the fp16
probabilities of the GPU may move a 2 to a 3).  The tests therefore assert the form of the MARKED rows, take the clean rows' form from last_row_forms(), and
require at least half of the clean reports and half of the clean anchors of each case in the default form."""
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LOGIT_TOL = 1e-3  # the project's contract (tests/test_gpu_parity.py LOGIT_TOL)
L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0)  # the peaked 2-layer model of tests/test_gpu_kernels.py
CASES = ("mid_all_80_3001", "mid_all_50_3002", "mid_cls_80_3003")


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def refs(golden_dir):
    return np.load(os.path.join(golden_dir, "guarded_form_refs.npz")), np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))


_inputs, _runs = {}, {}


def _mixed(refs, case):
    import make_guarded_form_refs as mg

    if case not in _inputs:
        _inputs.clear()
        _inputs[case] = mg.mixed_case(case, refs[1])
    return _inputs[case]


def _engine(dims, w, compute):
    from memvul_amd.binding import Engine

    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=16 * 512, max_batch=16, max_anchors=16)
    eng.load_state_dict(w, compute)
    return eng


def _run(refs, case, compute):
    """One fixture case through one engine: the 12 anchors appended one per call (each at the padded length of its own token count), the 16 reports through
    forward(ids, lens) at S = 256."""
    if (case, compute) not in _runs:
        dims, w, ids, lens, aids, alens, marked, amarked = _mixed(refs, case)
        eng = _engine(dims, w, compute)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # (the default form warns about the sink: tests/test_safe_form_gpu.py)
                aforms = []
                for g in range(len(alens)):
                    eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
                    aforms += eng.last_row_forms()
                out = eng.forward(ids, lens, want_embed=True)
            _runs[(case, compute)] = dict(logits=out["logits"], embed=out["embed"], bank=eng.anchor_get(), forms=eng.last_row_forms(), aforms=aforms,
                                          sat=eng.x8_saturation(), stats=eng.form_stats(), form=eng.form, marked=marked, amarked=amarked)
        finally:
            eng.close()
    return _runs[(case, compute)]


@pytest.mark.parametrize("case", CASES)
def test_guarded_form_holds_the_contract_and_flags_the_marked_sequences(gu, refs, case):
    """4. The contract on a batch in which half the sequences carry an ordinary-token sink; the marked reports and anchors come back in the safe form, at least
    half of the clean ones in the default form (a form that rescored everything would hold the contract for the wrong reason).  Measured maxima: DESIGN.md
    section 2 (diag record guarded_form_mixed)."""
    r = _run(refs, case, "guarded")
    err = np.abs(r["logits"] - refs[0][case + "_lg"])
    e = float(err.max())
    forms, aforms = np.array(r["forms"]), np.array(r["aforms"])
    clean, aclean = np.setdiff1d(np.arange(16), r["marked"]), np.setdiff1d(np.arange(12), r["amarked"])
    print(f"guarded form {case}: max |logit error| {e:.3e}; clean reports rescored {(forms[clean] == 'safe').sum()} of 8, clean anchors "
          f"{(aforms[aclean] == 'safe').sum()} of 6; form_stats {r['stats']}")
    gu.record("guarded_form_mixed", case=case, logits_err=e, err_marked_rows=float(err[r["marked"]].max()), err_clean_rows=float(err[clean].max()),
              clean_reports_rescored=int((forms[clean] == "safe").sum()), clean_anchors_rescored=int((aforms[aclean] == "safe").sum()), x8_saturation=r["sat"])
    assert r["form"] == "guarded"
    assert e <= LOGIT_TOL, e
    assert (forms[r["marked"]] == "safe").all() and (aforms[r["amarked"]] == "safe").all(), (forms, aforms)
    assert (forms[clean] == "default").sum() >= 4 and (aforms[aclean] == "default").sum() >= 3, (forms, aforms)
    assert r["sat"] == 0
    assert r["stats"] == (28, int((forms == "safe").sum() + (aforms == "safe").sum()))


def test_the_mixed_batch_tells_the_forms_apart(gu, refs):
    """4. On mid_all_80_3001 the default form on the same inputs exceeds the contract and reads more than twice the guarded maximum."""
    case = "mid_all_80_3001"
    e_g = float(np.abs(_run(refs, case, "guarded")["logits"] - refs[0][case + "_lg"]).max())
    d = _run(refs, case, "precise")
    e_d = float(np.abs(d["logits"] - refs[0][case + "_lg"]).max())
    print(f"{case} mixed batch: default {e_d:.3e} guarded {e_g:.3e}")
    gu.record("guarded_vs_default_form", case=case, err_default=e_d, err_guarded=e_g)
    assert d["form"] == "default" and set(d["forms"]) == {"default"}
    assert e_d > LOGIT_TOL and e_d > 2 * e_g, (e_d, e_g)


@pytest.mark.parametrize("case", CASES)
def test_each_row_has_the_bits_of_the_form_that_produced_it(gu, refs, case):
    """5. The same calls on a "safe" and on a "precise" engine: the rows last_row_forms() calls safe are byte-equal to the safe engine's, the others to the
    default form's; the same for the bank."""
    g, s, d = (_run(refs, case, c) for c in ("guarded", "safe", "precise"))
    assert set(s["forms"]) == {"safe"} and set(s["aforms"]) == {"safe"} and s["stats"] == (0, 0)
    for what, forms in (("embed", g["forms"]), ("bank", g["aforms"])):
        for i, f in enumerate(forms):
            assert g[what][i].tobytes() == (s if f == "safe" else d)[what][i].tobytes(), (what, i, f)


# ---- 6. every path ---------------------------------------------------------------------------------------------------------------------------------------------

def _ragged_batch(vocab):
    lens = np.array([16, 230, 40, 256, 64, 192, 100, 150, 128, 120, 200, 60, 256, 30, 180, 90], np.int32)
    ids, _ = synth.make_ids(len(lens), 256, vocab, seed=synth.SEED + 77, ragged=False)
    ids[ids == synth.MID_ID] = synth.MID_ID + 1
    ids = (ids * (np.arange(256)[None, :] < lens[:, None])).astype(np.int32)
    marked = np.arange(0, len(lens), 2)
    ids[marked] = synth.mark_mid_token(ids[marked], lens[marked])
    return np.ascontiguousarray(ids), lens, marked


def test_every_entry_point_rescores_the_flagged_rows(gu, refs):
    """6. A ragged batch (16 - 256 tokens, every other row marked) on mid_all_80_3001.  Entry points run a row at different padded lengths, so the comparison
    is per entry point: each gives, row by row, the bytes of the safe engine's result of the same call where the forms say safe and the default form's
    elsewhere; every marked row says safe; forward_by_length and its two halves agree byte for byte; form_stats() counts each sequence once per call."""
    dims, w, _, _, aids, alens, _, _ = _mixed(refs, "mid_all_80_3001")
    ids, lens, marked = _ragged_batch(dims.vocab_size)
    B = len(lens)
    bank = [0, 1, 6, 7]  # two marked anchors and the same two unmarked
    engs = {c: _engine(dims, w, c) for c in ("guarded", "safe", "precise")}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for eng in engs.values():
                for a in bank:
                    eng.anchor_append(aids[a:a + 1, :int(alens[a])], alens[a:a + 1])
            g, s, d = engs["guarded"], engs["safe"], engs["precise"]
            assert np.array_equal(g.anchor_get()[:2], s.anchor_get()[:2])

            def check(name, call, keys, forms_of=lambda: g.last_row_forms()):
                g.form_stats(reset=True)
                og = call(g)
                forms = np.array(forms_of())
                stats = g.form_stats()
                os_, od = call(s), call(d)
                print(f"{name}: rescored {int((forms == 'safe').sum())} of {B}")
                assert (forms[marked] == "safe").all(), (name, forms)
                assert stats == (B, int((forms == "safe").sum())), (name, stats)
                for k in keys:
                    for i in range(B):
                        want = os_ if forms[i] == "safe" else od
                        assert og[k][i].tobytes() == want[k][i].tobytes(), (name, k, i, forms[i])
                return og, forms

            # (the logits of a row depend on the bank as well, and the guarded bank mixes forms: rows are compared through their embeddings, and through the
            # matcher's outputs where the call has no embedding to give)
            check("forward", lambda e: e.forward(ids, lens, want_embed=True), ("embed",))
            check("encode", lambda e: {"embed": e.encode(ids, lens)}, ("embed",))
            whole, f_whole = check("forward_by_length", lambda e: e.forward_by_length(ids, lens, want_embed=True, min_tokens=1), ("embed",))

            def halves(e):
                t1 = e.forward_by_length_begin(ids, lens, want_embed=True, min_tokens=1)
                t2 = e.forward_by_length_begin(ids[::-1].copy(), lens[::-1].copy(), want_embed=True, min_tokens=1)
                assert t1[0] == "pending" and t2[0] == "pending"
                r1 = e.forward_by_length_end(t1)
                halves.forms1 = e.last_row_forms()
                r2 = e.forward_by_length_end(t2)
                assert np.array_equal(r2["embed"], r1["embed"][::-1])
                return r1

            g.form_stats(reset=True)
            r1 = halves(g)
            assert g.form_stats() == (2 * B, 2 * int((np.array(halves.forms1) == "safe").sum()))
            assert halves.forms1 == f_whole.tolist() and g.last_row_forms() == f_whole.tolist()[::-1]
            for k in ("logits", "probs", "best", "best_idx", "embed"):
                assert r1[k].tobytes() == whole[k].tobytes(), k
            rs, rd = halves(s), halves(d)
            for i in range(B):
                assert r1["embed"][i].tobytes() == (rs if f_whole[i] == "safe" else rd)["embed"][i].tobytes(), i

            # the resident sweep: the matcher's outputs against a bank of ONE form, so that a row's P(same) carries the row's form alone
            bank_safe = s.anchor_get()
            for eng in engs.values():
                eng.anchor_set(bank_safe)
            order = np.argsort(lens, kind="stable")
            for streams in (2, 1):
                for with_probs in (False, True):
                    for eng in engs.values():
                        eng.set_streams(streams)

                    def sweep(e):
                        best, idx, ps = e.bucketed_sweep(ids, lens, 4, with_probs=with_probs)
                        return {"best": best, "best_idx": idx, **({"ps": ps} if with_probs else {})}

                    def forms_of():
                        f = np.empty(B, object)
                        f[order] = g.corpus_row_forms(0, B)
                        return f.tolist()

                    check(f"bucketed_sweep streams={streams} with_probs={with_probs}", sweep, ("best", "best_idx") + (("ps",) if with_probs else ()), forms_of)
    finally:
        for eng in engs.values():
            eng.close()


# ---- 7. nothing flagged, nothing changed -----------------------------------------------------------------------------------------------------------------------

def test_nothing_flagged_nothing_changed(gu):
    """7. The bench's random-init 12-layer family (no item over 0.25 among millions): guarded outputs are byte-equal to the default form's through forward,
    forward_by_length and bucketed_sweep, nothing is rescored, and the global monitor counts the same."""
    dk, wk = dict(layers=12), dict()
    dims, w = gu.weights_for(dk, wk)
    kw = dict(max_tokens=32 * 256, max_batch=32, max_anchors=16)
    ids, lens = synth.make_ids(32, 256, dims.vocab_size, seed=synth.SEED + 5, ragged=True, min_len=20)
    aids, alens = synth.make_ids(8, 64, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=16)

    def run(eng):
        eng.anchor_reset()
        eng.attention_concentration(reset=True)
        eng.form_stats(reset=True)
        eng.anchor_append(aids, alens)
        out = {"bank": eng.anchor_get()}
        for k, v in eng.forward(ids, lens, want_embed=True).items():
            out["forward_" + k] = v
        for k, v in eng.forward_by_length(ids, lens, want_embed=True, min_tokens=1).items():
            out["by_length_" + k] = v
        out["sweep_best"], out["sweep_idx"], out["sweep_ps"] = eng.bucketed_sweep(ids, lens, 8, with_probs=True)
        conc = eng.attention_concentration()
        eng.anchor_reset()
        return out, conc

    d = gu.engine_for(dk, wk, compute_dtype="precise", **kw)
    od, conc_d = run(d)
    assert conc_d[1] == 0 and conc_d[2] > 0, conc_d  # the precondition: the default form sees no item over 0.25
    g = gu.engine_for(dk, wk, compute_dtype="guarded", **kw)
    assert g.form == "guarded"
    og, conc_g = run(g)
    for k in od:
        assert og[k].tobytes() == od[k].tobytes(), k
    assert g.form_stats() == (8 + 3 * 32, 0)
    assert conc_g == conc_d
    assert set(g.corpus_row_forms(0, 32)) == {"default"}


# ---- 8. the rule where the monitor fires on part of the items --------------------------------------------------------------------------------------------------

def test_the_rule_on_the_peaky_two_layer_model(gu):
    """8. L2 / WK of tests/test_safe_form_gpu.py (one monitored layer: 12 items per sequence, rescored at >= 1): whatever subset the rule flags, each row's
    embedding is byte-equal to the engine of the form last_row_forms() names."""
    dims, w = gu.weights_for(L2, WK)
    ids, lens = synth.make_ids(16, 256, dims.vocab_size, seed=synth.SEED + 9, ragged=True, min_len=12)
    lens[:2] = (8, 12)  # two sequences the monitor does not look at: they stay in the default form whatever their heads do
    ids = np.ascontiguousarray(ids * (np.arange(256)[None, :] < lens[:, None]), np.int32)
    kw = dict(max_tokens=16 * 256, max_batch=16, max_anchors=16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = gu.engine_for(L2, WK, compute_dtype="guarded", **kw)
        g.form_stats(reset=True)
        eg = g.encode(ids, lens)
        forms = g.last_row_forms()
        stats = g.form_stats()
        es = gu.engine_for(L2, WK, compute_dtype="safe", **kw).encode(ids, lens)
        ed = gu.engine_for(L2, WK, compute_dtype="precise", **kw).encode(ids, lens)
    n_safe = sum(f == "safe" for f in forms)
    print(f"peaky 2-layer model: {n_safe} of 16 rows rescored")
    gu.record("guarded_form_peaky_l2", rescored=n_safe, rows=16)
    assert stats == (16, n_safe)
    for i, f in enumerate(forms):
        assert eg[i].tobytes() == (es if f == "safe" else ed)[i].tobytes(), (i, f)
        assert (f == "default") if int(lens[i]) < 16 else True, (i, int(lens[i]))  # the monitor does not look at a sequence of fewer than 16 tokens


# ---- 9. strictness ---------------------------------------------------------------------------------------------------------------------------------------------

def test_the_guarded_form_is_a_form_of_the_precise_dtype(gu, monkeypatch):
    from memvul_amd.binding import Engine

    dims, w = gu.weights_for(L2, WK)
    kw = dict(vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=4096, max_batch=16, max_anchors=16)
    monkeypatch.setenv("MEMVUL_FORM", "guarded")
    eng = Engine(0, **kw)
    try:
        with pytest.raises(RuntimeError, match="MEMVUL_FORM"):
            eng.load_state_dict(w, "f16")
    finally:
        eng.close()
    eng = Engine(0, **kw)
    try:
        eng.load_state_dict(w, "precise")
        assert eng.form == "guarded"  # the switch alone selects the form: how bench.py measures it
    finally:
        eng.close()
    monkeypatch.delenv("MEMVUL_FORM")
    eng = Engine(0, **kw)
    try:
        eng.load_state_dict(w, "f16")
        with pytest.raises(RuntimeError, match="MV_F16"):
            eng.set_form("guarded")
        assert eng.form == "default"
    finally:
        eng.close()
