"""The safe form of MV_F16X8 (include/memvul_hip.h mv_set_form), the parts that need no GPU: the ABI moved in all three places, the host logic of the
MEMVUL_ON_SINK fall-back (binding.Engine) against a stand-in library, and the float64 rounding model's price of the form."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3


def test_header_binding_and_library_carry_the_form():
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    for name in ("mv_set_form", "mv_get_form"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in binding.ABI_SYMBOLS
    assert re.search(r"#define MV_FORM_DEFAULT 0\b", hdr) and re.search(r"#define MV_FORM_SAFE 1\b", hdr)
    assert (binding.MV_FORM_DEFAULT, binding.MV_FORM_SAFE) == (0, 1)
    lib = binding.load_library()
    assert lib.mv_set_form.argtypes == [C.c_void_p, C.c_int] and lib.mv_get_form.argtypes == [C.c_void_p]
    assert binding.compute_dtype_of("safe") == binding.MV_F16X8
    assert binding.wants_safe_form("safe") and not binding.wants_safe_form("precise") and not binding.wants_safe_form(binding.MV_F16X8)
    assert "MEMVUL_FORM" in hdr and "six" in hdr[hdr.index("Environment switches read HERE"):][:200]


# ---- the fall-back's host logic ----------------------------------------------------------------------------------------------------------------------------------

class _Quick:
    def __init__(self, lib):
        self.lib = lib

    def mv_anchor_count(self, h):
        return self.lib.n_anchors

    def mv_x8_saturation(self, h, n, reset):
        n._obj.value = self.lib.saturated
        return 0

    def mv_attention_concentration(self, h, m, n, t, reset):
        self.lib.log.append(("concentration", bool(reset)))
        m._obj.value, n._obj.value, t._obj.value = (0.64 if self.lib.over else 0.0), self.lib.over, self.lib.total
        if reset:
            self.lib.over = self.lib.total = 0
        return 0


class _Lib:
    """What binding.Engine calls of libmemvul_hip.so, as a recorder: every pass-like call adds `items` (sequence, head, layer) items to the monitor, `sink_share`
    of them over the threshold, and writes the form it ran in into its first output value.  `saturated`: what mv_x8_saturation counts; `begin_rc`: what
    mv_forward_ragged_begin answers instead of taking the batch (-5: MV_ERR_CAPACITY)."""

    def __init__(self, items=200, sink_share=0.5, saturated=0, begin_rc=0):
        self.form, self.log, self.n_anchors, self.over, self.total = 0, [], 0, 0, 0
        self.items, self.sink_share, self.saturated, self.begin_rc = items, sink_share, saturated, begin_rc
        self.quick = _Quick(self)
        self.next_ticket, self.in_flight = 0, {}

    def _pass(self):
        self.total += self.items
        self.over += int(self.items * self.sink_share)

    def _stamp(self, best):
        C.cast(best, C.POINTER(C.c_float))[0] = float(self.form)

    def mv_set_form(self, h, form):
        self.log.append(("set_form", form))
        self.form = form
        return 0

    def mv_get_form(self, h):
        return self.form

    def mv_anchor_reset(self, h):
        self.log.append(("anchor_reset",))
        self.n_anchors = 0
        return 0

    def mv_anchor_append(self, h, ids, lens, n, S):
        self.log.append(("anchor_append", n, S, self.form))
        self.n_anchors += n
        self._pass()
        return 0

    def mv_anchor_set(self, h, v, G):
        self.log.append(("anchor_set", G))
        self.n_anchors = G
        return 0

    def mv_forward(self, h, ids, lens, B, S, logits, probs, best, idx, embed):
        self.log.append(("forward", self.form))
        self._pass()
        self._stamp(best)
        return 0

    def mv_forward_ragged(self, h, ids, lens, B, S, mt, logits, probs, best, idx, embed):
        self.log.append(("ragged", self.form))
        self._pass()
        self._stamp(best)
        return 0

    def mv_forward_ragged_begin(self, h, ids, lens, B, S, mt, wl, wp, we, ticket):
        if self.begin_rc:
            self.log.append(("begin_refused", self.begin_rc))
            return self.begin_rc
        t = self.next_ticket
        self.next_ticket += 1
        self.in_flight[t] = self.form
        ticket._obj.value = t
        self.log.append(("begin", t, self.form))
        self._pass()
        return 0

    def mv_forward_ragged_end(self, h, t, logits, probs, best, idx, embed):
        self.log.append(("end", t))
        C.cast(best, C.POINTER(C.c_float))[0] = float(self.in_flight.pop(t))
        return 0

    def mv_corpus_upload(self, h, ids, lens, n, S):
        self.log.append(("upload", n, S))
        return 0

    def mv_corpus_run_len(self, h, first, count, batch, keep, s_eff):
        self.log.append(("run", first, count, s_eff, self.form))
        self.swept = self.form
        self._pass()
        return 0

    def mv_corpus_results(self, h, first, count, best, idx, ps):
        self.log.append(("results", first, count))
        C.cast(best, C.POINTER(C.c_float))[0] = float(self.swept)
        return 0

    def mv_encode(self, h, ids, lens, B, S, out):
        self.log.append(("encode", self.form))
        self._pass()
        self._stamp(out)
        return 0

    def mv_match(self, h, u, B, logits, probs, best, idx):
        self.log.append(("match", B))
        self._stamp(best)
        return 0


class StandInEngine(binding.Engine):
    """binding.Engine's host logic on the recorder above (no GPU, no library)."""

    def __init__(self, lib):
        self._lib, self._h, self.P, self._tickets = lib, None, 512, []
        self._precise, self._sat_warned = True, False
        self._init_sink_state()

    def close(self):
        pass


IDS = np.arange(8 * 256, dtype=np.int32).reshape(8, 256) % 1000 + 5
LENS = np.full(8, 256, np.int32)


def _told(rec, needle):
    return [str(r.message) for r in rec if needle in str(r.message)]


def test_policy_is_parsed_strictly(monkeypatch):
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    assert binding.on_sink_policy() == "warn"
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    assert binding.on_sink_policy() == "safe"
    for bad in ("maybe", "SAFE", "", "1"):
        monkeypatch.setenv("MEMVUL_ON_SINK", bad)
        with pytest.raises(ValueError, match="MEMVUL_ON_SINK"):
            binding.on_sink_policy()


def test_trip_switches_once_redoes_the_call_and_keeps_an_installed_bank(monkeypatch):
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    lib = _Lib()
    eng = StandInEngine(lib)
    eng.anchor_set(np.zeros((5, 512), np.float32))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = eng.forward(IDS, LENS)
        out2 = eng.forward(IDS, LENS)
        emb = eng.encode(IDS, LENS)
    assert eng.form == "safe" and out["best"][0, 0] == 1.0 and out2["best"][0, 0] == 1.0 and emb[0, 0] == 1.0
    told = _told(rec, "SAFE form")
    assert len(told) == 1 and "KEPT" in told[0]
    # the call in the default form, the monitor read, the switch, the counters reset, the call again — and nothing but plain calls afterwards
    assert lib.log == [("anchor_set", 5), ("forward", 0), ("concentration", False), ("set_form", 1), ("concentration", True), ("forward", 1), ("forward", 1),
                       ("encode", 1)]


def test_trip_in_anchor_append_encodes_the_whole_bank_again(monkeypatch):
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    lib = _Lib(items=60)  # the first append stays below 100 items: no verdict yet
    eng = StandInEngine(lib)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.anchor_append(IDS[:3], LENS[:3])
        assert eng.form == "default"
        eng.anchor_append(IDS[3:5, :128], LENS[3:5] // 2)
    assert eng.form == "safe" and eng.n_anchors == 5
    assert len(_told(rec, "SAFE form")) == 1 and "encoded again" in _told(rec, "SAFE form")[0]
    tail = lib.log[lib.log.index(("set_form", 1)):]
    assert tail == [("set_form", 1), ("concentration", True), ("anchor_reset",), ("anchor_append", 3, 256, 1), ("anchor_append", 2, 128, 1)]
    # anchor_reset forgets the ids; anchors appended in the safe form are not kept
    eng.anchor_reset()
    eng.anchor_append(IDS[:2], LENS[:2])
    assert eng._anchor_log == []


def test_no_trip_below_the_condition_and_none_in_the_safe_form(monkeypatch):
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    for lib in (_Lib(items=99, sink_share=1.0), _Lib(items=1000, sink_share=0.02)):  # fewer than 100 items; not MORE than 2 %
        eng = StandInEngine(lib)
        eng.anchor_set(np.zeros((2, 512), np.float32))
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            eng.forward(IDS, LENS)
        assert eng.form == "default" and not rec and ("set_form", 1) not in lib.log
    lib = _Lib()
    eng = StandInEngine(lib)
    eng.set_form("safe")
    eng.anchor_set(np.zeros((2, 512), np.float32))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.forward(IDS, LENS)
    assert not rec and [c for c in lib.log if c[0] == "concentration"] == []  # the safe form trips nothing (the library keeps counting)


def test_tickets_begun_before_the_trip_are_scored_again_in_order(monkeypatch):
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    lib = _Lib()
    eng = StandInEngine(lib)
    eng.anchor_set(np.zeros((2, 512), np.float32))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        t1 = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
        t2 = eng.forward_by_length_begin(IDS[::-1].copy(), LENS, min_tokens=256)
        assert t1[0] == t2[0] == "pending" and eng.form == "default"
        r1 = eng.forward_by_length_end(t1)
        assert eng.form == "safe"
        r2 = eng.forward_by_length_end(t2)
        t3 = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)  # begun in the safe form: nothing kept, nothing redone
        r3 = eng.forward_by_length_end(t3)
    assert len(_told(rec, "SAFE form")) == 1
    assert r1["best"][0, 0] == r2["best"][0, 0] == r3["best"][0, 0] == 1.0
    assert t3[-1] is None
    assert lib.log == [("anchor_set", 2), ("begin", 0, 0), ("begin", 1, 0), ("end", 0), ("concentration", False), ("set_form", 1), ("concentration", True),
                       ("ragged", 1), ("end", 1), ("ragged", 1), ("begin", 2, 1), ("end", 2)]


def test_the_resident_sweep_runs_once_more_after_a_trip(monkeypatch):
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    lib = _Lib()
    eng = StandInEngine(lib)
    eng.anchor_set(np.zeros((2, 512), np.float32))
    lens = np.array([30, 200, 60, 256, 100, 130, 250, 40], np.int32)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        best, idx, _ = eng.bucketed_sweep(IDS, lens, 4)
        eng.bucketed_sweep(IDS, lens, 4)
    assert len(_told(rec, "SAFE form")) == 1 and eng.form == "safe"
    assert best[np.argsort(lens, kind="stable")[0], 0] == 1.0  # (the recorder stamps the first sorted row: the results handed out are the second sweep's)
    first = [("upload", 8, 256), ("run", 0, 4, 100, 0), ("run", 4, 4, 256, 0), ("results", 0, 8), ("concentration", False), ("set_form", 1), ("concentration", True),
             ("run", 0, 4, 100, 1), ("run", 4, 4, 256, 1), ("results", 0, 8)]
    assert lib.log[1:] == first + [("upload", 8, 256), ("run", 0, 4, 100, 1), ("run", 4, 4, 256, 1), ("results", 0, 8)]


def test_warn_is_todays_behaviour(monkeypatch):
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    lib = _Lib()
    eng = StandInEngine(lib)
    eng.anchor_set(np.zeros((2, 512), np.float32))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = eng.forward(IDS, LENS)
        eng.forward(IDS, LENS)
        t = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
        eng.forward_by_length_end(t)
    told = _told(rec, "ONE ordinary token")
    assert len(told) == 1 and "MEMVUL_CLS_ASIDE=0 MEMVUL_QKV_ASIDE=qkv is the most conservative form" in told[0]
    assert eng.form == "default" and out["best"][0, 0] == 0.0 and not [c for c in lib.log if c[0] == "set_form"]
    assert t[-1] is None and eng._anchor_log == []  # nothing is kept for a switch that cannot happen


# ---- the float64 model prices the form --------------------------------------------------------------------------------------------------------------------------

def test_the_rounding_model_prices_the_safe_form(golden_dir):
    """oracle/precision_model.py on mid_all_80_3001 (stored gains, 3 issue reports x 3 anchors): both terms everywhere leaves 1.35e-3 (the GPU measured 1.40e-3 for
    MEMVUL_CLS_ASIDE=0 MEMVUL_QKV_ASIDE=qkv on the same case) — what is left is the single-plane fp16 storage of Q, K, V, P inside attention — and two planes
    there bring it to 9.5e-5.  The argument the safe form rests on."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import r06_make_sink_refs as mk6
    from memvul_amd import synth
    from oracle import precision_model as pm

    refs = np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))
    dims, w, ids, lens, aids, alens, _ = mk6.case("mid", "all", 0.8, 3001, gains=refs["mid_all_80_3001_gains"])
    ids, lens, aids, alens = ids[:3], lens[:3], aids[:3], alens[:3]
    LA = int(alens.max())
    aids = aids[:, :LA]
    mask, amask = synth.mask_from_lens(lens, ids.shape[1]), synth.mask_from_lens(alens, LA)
    ref = pm.logits(w, ids, mask, aids, amask, None)[0]
    both = dict(pm.X8_ENGINE, a_qkv="f16x8")
    e_one = float(np.abs(pm.logits(w, ids, mask, aids, amask, pm.engine_formats(12, "f16", **both))[0] - ref).max())
    e_two = float(np.abs(pm.logits(w, ids, mask, aids, amask, pm.engine_formats(12, "f16", **dict(both, qkv="f16x2", p="f16x2")))[0] - ref).max())
    print(f"model, mid_all_80_3001: both terms everywhere {e_one:.2e}, + two planes of Q, K, V, P {e_two:.2e}")
    assert e_two <= 0.5 * LOGIT_TOL, e_two
    assert e_one > LOGIT_TOL, e_one
