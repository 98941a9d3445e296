"""The guarded form of MV_F16X8 (include/memvul_hip.h MV_FORM_GUARDED), the parts that need no GPU: the ABI in all three places, the host logic of
binding.Engine in that form against a stand-in library, and the float64 rounding model's price of the per-sequence rule."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_safe_form_cpu as sf  # noqa: E402  (the recorder library and the stand-in engine)

LOGIT_TOL = 1e-3


def test_header_binding_and_library_carry_the_guarded_form():
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    assert re.search(r"#define MV_FORM_GUARDED 2\b", hdr) and binding.MV_FORM_GUARDED == 2 and binding.FORMS["guarded"] == 2
    for name in ("mv_form_stats", "mv_last_row_forms", "mv_corpus_row_forms"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in binding.ABI_SYMBOLS
    lib = binding.load_library()
    i64p = C.POINTER(C.c_int64)
    assert lib.mv_form_stats.argtypes == [C.c_void_p, i64p, i64p, C.c_int] and lib.mv_form_stats.restype == C.c_int
    assert lib.mv_last_row_forms.argtypes == [C.c_void_p, C.c_void_p, C.c_int]
    assert lib.mv_corpus_row_forms.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    assert binding.compute_dtype_of("guarded") == binding.MV_F16X8 and binding.wanted_form("guarded") == "guarded" and binding.wanted_form("precise") is None
    assert not binding.wants_safe_form("guarded")
    # a new VALUE of MEMVUL_FORM, not a seventh switch
    env = hdr[hdr.index("Environment switches read HERE"):]
    assert "six" in env[:200] and re.search(r"MEMVUL_FORM\s+default \| safe \| guarded", env)
    # every int mv_* is a function-try-block
    from stage_kit import host_source

    src = host_source()
    for name in ("mv_form_stats", "mv_last_row_forms", "mv_corpus_row_forms"):
        assert re.search(r"\nint %s\([^)]*\) try \{" % name, src), name


# ---- the host logic ---------------------------------------------------------------------------------------------------------------------------------------------

class _Quick(sf._Quick):
    def mv_form_stats(self, h, n, r, reset):
        self.lib.log.append(("form_stats",))
        n._obj.value, r._obj.value = self.lib.seqs, self.lib.rescored
        return 0


class _Lib(sf._Lib):
    """The recorder of test_safe_form_cpu.py + the guarded form's counters: every pass-like call adds `rows` sequences, `flag_share` of them rescored."""

    def __init__(self, rows=200, flag_share=0.5, **kw):
        super().__init__(**kw)
        self.quick = _Quick(self)
        self.rows, self.flag_share, self.seqs, self.rescored = rows, flag_share, 0, 0

    def _pass(self):
        super()._pass()
        if self.form == binding.MV_FORM_GUARDED:
            self.seqs += self.rows
            self.rescored += int(self.rows * self.flag_share)

    def _row_forms(self, out, n):
        for r in range(n):  # (every third row "safe": the decoding is visible)
            C.cast(out, C.POINTER(C.c_uint8))[r] = binding.MV_FORM_SAFE if r % 3 == 1 else binding.MV_FORM_DEFAULT
        return 0

    def mv_last_row_forms(self, h, out, n):
        self.log.append(("last_row_forms", n))
        return self._row_forms(out, n)

    def mv_corpus_row_forms(self, h, first, count, out):
        self.log.append(("corpus_row_forms", first, count))
        return self._row_forms(out, count)


def _guarded_engine(lib):
    eng = sf.StandInEngine(lib)
    eng.set_form("guarded")
    eng.anchor_set(np.zeros((2, 512), np.float32))
    return eng


@pytest.mark.parametrize("policy", ["warn", "safe"])
def test_no_trip_and_no_sink_warning_in_the_guarded_form(monkeypatch, policy):
    monkeypatch.setenv("MEMVUL_ON_SINK", policy)
    lib = _Lib(items=1000, sink_share=1.0, flag_share=0.0)  # the monitor says "sink" in every item
    eng = _guarded_engine(lib)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = eng.forward(sf.IDS, sf.LENS)
        eng.encode(sf.IDS, sf.LENS)
        eng.anchor_append(sf.IDS[:2], sf.LENS[:2])
        t = eng.forward_by_length_begin(sf.IDS, sf.LENS, min_tokens=256)
        eng.forward_by_length_end(t)
        eng.bucketed_sweep(sf.IDS, sf.LENS, 4)
    assert not rec, [str(r.message) for r in rec]
    assert eng.form == "guarded" and out["best"][0, 0] == float(binding.MV_FORM_GUARDED)
    assert [c for c in lib.log if c[0] == "set_form"] == [("set_form", binding.MV_FORM_GUARDED)]
    assert not [c for c in lib.log if c[0] == "concentration"]  # the guarded form answers per sequence: the global counters trip nothing
    assert t[-1] is None and eng._corpus_runs == []  # no ticket and no sweep is kept to be scored again: nothing switches the form under them


def test_one_warning_above_a_quarter_rescored_and_none_at_or_below(monkeypatch):
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    for lib in (_Lib(rows=200, flag_share=0.25), _Lib(rows=99, flag_share=1.0), _Lib(rows=200, flag_share=0.0)):  # not MORE than a quarter; fewer than 100 seen
        eng = _guarded_engine(lib)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            eng.forward(sf.IDS, sf.LENS)
        assert not rec, [str(r.message) for r in rec]
    lib = _Lib(rows=200, flag_share=0.26)
    eng = _guarded_engine(lib)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.forward(sf.IDS, sf.LENS)
        eng.forward(sf.IDS, sf.LENS)
        eng.encode(sf.IDS, sf.LENS)
    told = sf._told(rec, "guarded form")
    assert len(told) == 1 and len(rec) == 1 and "52 of 200" in told[0] and "safe" in told[0]
    assert eng.form == "guarded"  # it says so once and keeps rescoring: a row's bits do not depend on what the handle saw before
    assert [c for c in lib.log if c[0] == "form_stats"] == [("form_stats",)]  # (not read again once it has warned)


def test_the_names_are_parsed_strictly(monkeypatch):
    assert binding.compute_dtype_of("guarded") == binding.MV_F16X8 and binding.compute_dtype_of("GUARDED") == binding.MV_F16X8
    with pytest.raises(ValueError, match="unknown compute dtype"):
        binding.compute_dtype_of("guardd")
    monkeypatch.setenv("MEMVUL_COMPUTE", "guarded")
    assert binding.wanted_form(None) == "guarded" and binding.compute_dtype_of(None) == binding.MV_F16X8
    eng = sf.StandInEngine(_Lib())
    with pytest.raises(ValueError, match="unknown form"):
        eng.set_form("guardd")
    assert eng.form == "default"
    eng.set_form("guarded")
    assert eng.form == "guarded"
    eng.set_form("default")
    assert eng.form == "default"


# ---- the float64 model prices the rule --------------------------------------------------------------------------------------------------------------------------

def test_the_rounding_model_prices_the_per_sequence_rule(golden_dir):
    """oracle/precision_model.py on mid_all_80_3001 (stored gains): four 256-token reports, rows 0 - 1 with the sink token, rows 2 - 3 with every MID_ID replaced
    by MID_ID + 1, two anchors that carry the sink.  The monitor's items (the exact forward's [CLS] row, keys other than [CLS] / [SEP]; 144 per sequence: the
    model prunes nothing) separate the two kinds of sequence, and "flagged -> safe form, else default form; the bank likewise" prices at 2.6e-4 where the
    default form on both sides reads 1.6 - 1.8e-3."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import r06_make_sink_refs as mk6
    from memvul_amd import synth
    from oracle import concentration as conc
    from oracle import memvul_oracle as orc
    from oracle import precision_model as pm

    refs = np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))
    dims, w, ids, lens, aids, alens, _ = mk6.case("mid", "all", 0.8, 3001, gains=refs["mid_all_80_3001_gains"])
    ids, lens, aids, alens = ids[:4].copy(), lens[:4], aids[:2], alens[:2]
    for b in (2, 3):
        ids[b][ids[b] == synth.MID_ID] = synth.MID_ID + 1
    LA = int(alens.max())
    aids = aids[:, :LA]
    mask, amask = synth.mask_from_lens(lens, ids.shape[1]), synth.mask_from_lens(alens, LA)

    def items_over(I, L, M):
        """(exact embeddings, items over 0.25 per sequence): oracle/concentration.py, a recording format in the place of P's rounding, for the length of this call."""
        coll, u = conc.cls_collision(w, I, L, forward=pm.instance_forward, with_output=True)
        assert coll.shape == (12, len(L), 12) and np.array_equal(conc.orc_mask(L, I.shape[1]), M)
        return u, (coll > 0.25).sum(axis=(0, 2))

    u_ref, over = items_over(ids, lens, mask)
    v_ref, a_over = items_over(aids, alens, amask)
    print("items over 0.25 of 144: reports", over.tolist(), "anchors", a_over.tolist())
    assert (over[:2] >= 100).all() and (over[2:] == 0).all(), over
    flagged, a_flagged = over > 0.02 * 144, a_over > 0.02 * 144
    assert flagged.tolist() == [True, True, False, False] and a_flagged.all()

    Wm = w["_projector.weight"].astype(np.float64)
    ref = orc.match(u_ref, v_ref, Wm)[0]
    default = lambda: pm.engine_formats(12, "f16", **pm.X8_ENGINE_SHIPPED)  # noqa: E731
    safe = lambda: pm.engine_formats(12, "f16", **dict(pm.X8_ENGINE, a_qkv="f16x8", qkv="f16x2", p="f16x2"))  # noqa: E731
    u_def = pm.instance_forward(w, ids, mask, default(), **pm.SHIPPED_KW)
    u_safe = pm.instance_forward(w, ids, mask, safe())
    v_def = pm.instance_forward(w, aids, amask, default(), **pm.SHIPPED_KW)
    v_safe = pm.instance_forward(w, aids, amask, safe())

    def err(u, v):
        return np.abs(orc.match(u, v, Wm)[0] - ref).max(axis=(1, 2))

    e_def = err(u_def, v_def)
    e_guard = err(np.where(flagged[:, None], u_safe, u_def), np.where(a_flagged[:, None], v_safe, v_def))
    print("model, mid_all_80_3001 mixed batch: default x default bank", e_def, " per-sequence rule", e_guard)
    assert (e_guard <= 0.5 * LOGIT_TOL).all(), e_guard
    assert (e_def > LOGIT_TOL).all(), e_def
