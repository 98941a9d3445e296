"""The host logic of binding.Engine as a trace: what tests/test_binding_trace_cpu.py holds a rewrite of memvul_amd/binding.py to.

Every scenario drives a fresh binding.Engine (tests/test_safe_form_cpu.py StandInEngine) on the recorder libraries of the CPU tests, composed by inheritance
(Recorder), and records: the recorder's log, the library entries in the order they were called, every warning (category, text, whether it is attributed to THIS
file: every public method is called from here, so a warning of a direct call must be), every exception (type, text), the stamps the recorder wrote into the
results, and the engine's state at the end.  No GPU and no built library.

  python scripts/binding_trace.py --out tests/golden/binding_trace.json     (at the commit whose behaviour is to be pinned)"""
import contextlib
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_corpus_rematch_cpu as rm  # noqa: E402
import test_safe_form_cpu as sf  # noqa: E402
import test_sink_routing_cpu as sr  # noqa: E402  (its recorder extends the guarded form's)

from memvul_amd import binding  # noqa: E402

HERE = os.path.abspath(__file__)
ENV = ("MEMVUL_ON_SINK", "MEMVUL_SINK_CENSUS", "MEMVUL_SINK_TOKENS", "MEMVUL_TOKENIZE", "MEMVUL_COMPUTE")
IDS, LENS = sf.IDS, sf.LENS
RAGGED = rm.LENS


class Recorder(sr._Lib, rm._Lib):
    """Every entry any of the four recorders implements, in one library."""


def entries(lib) -> set:
    return {n for obj in (lib, lib.quick) for n in dir(obj) if n.startswith("mv_")}


def bank(n):
    return np.zeros((n, 512), np.float32)


class Trace:
    """One scenario's record.  ``with t.call(label):`` runs one step: an exception ends the step and is recorded, the warnings it raised are recorded under its
    label; via = the public method a step goes through before it reaches the one that warns (None: a direct call)."""

    def __init__(self, **lib_kw):
        self.lib = Recorder(**lib_kw)
        self.calls, self.rec = [], {"warnings": [], "errors": [], "stamps": {}}
        for obj in (self.lib, self.lib.quick):
            for name in [n for n in dir(obj) if n.startswith("mv_")]:
                setattr(obj, name, self._named(getattr(obj, name), name))
        self.tickets = {}

    def _named(self, fn, name):
        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call

    def engine(self):
        return sf.StandInEngine(self.lib)

    @contextlib.contextmanager
    def call(self, label, via=None):
        with warnings.catch_warnings(record=True) as got:
            warnings.simplefilter("always")
            try:
                yield
            except Exception as e:  # noqa: BLE001  (the type and the text are the record)
                self.rec["errors"].append({"step": label, "type": type(e).__name__, "text": str(e)})
        for w in got:
            self.rec["warnings"].append({"step": label, "via": via, "category": w.category.__name__, "text": str(w.message),
                                         "from_scenario_file": os.path.abspath(w.filename) == HERE})

    def stamp(self, label, value):
        self.rec["stamps"][label] = value if isinstance(value, (list, str, int)) else float(value)

    def done(self, eng=None) -> dict:
        out = dict(self.rec, log=[list(c) for c in self.lib.log], calls=self.calls)
        if eng is not None:
            out["end"] = {"form": eng.form, "n_anchors": eng.n_anchors, "anchor_log": len(eng._anchor_log), "corpus_runs": len(eng._corpus_runs),
                          "tickets": list(eng._tickets), "held": {k: [t[0], t[1] if isinstance(t[1], int) else sorted(t[1]), t[-1] is None] for k, t in sorted(self.tickets.items())}}
        return out


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


# ---- the entry points that read the monitors, each called from this file ----------------------------------------------------------------------------------------

def via_forward(t, eng):
    with t.call("forward"):
        t.stamp("forward", eng.forward(IDS, LENS)["best"][0, 0])


def via_encode(t, eng):
    with t.call("encode"):
        t.stamp("encode", eng.encode(IDS, LENS)[0, 0])


def via_anchor_append(t, eng):
    with t.call("anchor_append"):
        eng.anchor_append(IDS[:3], LENS[:3])


def via_by_length(t, eng):
    with t.call("forward_by_length"):
        t.stamp("forward_by_length", eng.forward_by_length(IDS, LENS, min_tokens=256)["best"][0, 0])


def via_by_length_small(t, eng):
    with t.call("forward_by_length below min_tokens", via="forward"):
        t.stamp("forward_by_length below min_tokens", eng.forward_by_length(IDS, LENS)["best"][0, 0])


def via_by_length_end(t, eng):
    with t.call("forward_by_length_begin"):
        t.tickets["t"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
    with t.call("forward_by_length_end"):
        t.stamp("forward_by_length_end", eng.forward_by_length_end(t.tickets["t"])["best"][0, 0])


def via_corpus_results(t, eng):
    with t.call("corpus_upload + corpus_run"):
        eng.corpus_upload(IDS, LENS)
        eng.corpus_run(0, 8, 8)
    with t.call("corpus_results"):
        t.stamp("corpus_results", eng.corpus_results(0, 8)[0][0, 0])


def via_bucketed_sweep(t, eng):
    with t.call("bucketed_sweep", via="corpus_results"):
        best, idx, ps = eng.bucketed_sweep(IDS, RAGGED, 4)
        t.stamp("bucketed_sweep", best[:, 0].tolist())


ENTRY_POINTS = {"forward": via_forward, "encode": via_encode, "anchor_append": via_anchor_append, "forward_by_length": via_by_length,
                "forward_by_length_small": via_by_length_small, "forward_by_length_end": via_by_length_end, "corpus_results": via_corpus_results,
                "bucketed_sweep": via_bucketed_sweep}


# ---- the scenarios ----------------------------------------------------------------------------------------------------------------------------------------------

def s1_default_form():
    """MEMVUL_ON_SINK unset, the default form, every entry point once (the recorder reports a sink in half the items: the first read warns, once)."""
    t = Trace()
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(3))
    via_forward(t, eng)
    with t.call("forward again"):
        t.stamp("forward again", eng.forward(IDS, LENS, want_logits=False, want_embed=True)["best"][0, 0])
    via_by_length(t, eng)
    via_by_length_small(t, eng)
    via_by_length_end(t, eng)
    via_encode(t, eng)
    with t.call("anchor_append"):
        eng.anchor_append(IDS[:2], LENS[:2])
    via_bucketed_sweep(t, eng)
    with t.call("corpus_results"):
        best, idx, ps = eng.corpus_results(0, 8, with_probs=True)
        t.stamp("corpus_results", [best[:, 0].tolist(), idx.tolist(), list(ps.shape)])
    with t.call("match"):
        out = eng.match(bank(4))
        t.stamp("match", [sorted(out), [list(out[k].shape) for k in sorted(out)], [out[k].dtype.str for k in sorted(out)]])
    with t.call("anchor_reset"):
        eng.anchor_reset()
    return t.done(eng)


def s1_warning_from(entry):
    """MEMVUL_ON_SINK unset: the one sink warning, raised by `entry` as the first call that reads the monitor."""
    t = Trace()
    eng = t.engine()
    ENTRY_POINTS[entry](t, eng)
    via_forward(t, eng)  # (says nothing again)
    return t.done(eng)


def s2_trip_from(entry):
    """MEMVUL_ON_SINK=safe: `entry` trips, over a bank installed with anchor_set (kept)."""
    t = Trace()
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(5))
    ENTRY_POINTS[entry](t, eng)
    via_forward(t, eng)
    via_encode(t, eng)
    return t.done(eng)


def s2_trip_in_anchor_append_replays_the_bank():
    t = Trace(items=60)  # (the first append stays below 100 items)
    eng = t.engine()
    with t.call("anchor_append 3"):
        eng.anchor_append(IDS[:3], LENS[:3])
    t.stamp("form after the first append", eng.form)
    with t.call("anchor_append 2"):
        eng.anchor_append(IDS[3:5, :128], LENS[3:5] // 2)
    with t.call("anchor_reset + anchor_append in the safe form"):
        eng.anchor_reset()
        eng.anchor_append(IDS[:2], LENS[:2])
    return t.done(eng)


def s2_trip_with_an_empty_installed_bank():
    t = Trace()
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(0))
    via_encode(t, eng)
    return t.done(eng)


def s2_trip_with_two_tickets_in_flight():
    t = Trace()
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    with t.call("begin 1, 2"):
        t.tickets["t1"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
        t.tickets["t2"] = eng.forward_by_length_begin(IDS[::-1].copy(), LENS, want_probs=False, min_tokens=256)
    with t.call("forward_by_length_end 1"):
        t.stamp("end 1", eng.forward_by_length_end(t.tickets["t1"])["best"][0, 0])
    with t.call("forward_by_length_end 2", via="forward_by_length"):
        out = eng.forward_by_length_end(t.tickets["t2"])
        t.stamp("end 2", [float(out["best"][0, 0]), out["probs"] is None])
    with t.call("begin 3"):
        t.tickets["t3"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
    with t.call("forward_by_length_end 3"):
        t.stamp("end 3", eng.forward_by_length_end(t.tickets["t3"])["best"][0, 0])
    return t.done(eng)


def s2_trip_inside_a_done_ticket():
    t = Trace(begin_rc=-5)
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    with t.call("forward_by_length_begin", via="forward_by_length"):
        t.tickets["t"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
    with t.call("forward_by_length_end"):
        t.stamp("end", eng.forward_by_length_end(t.tickets["t"])["best"][0, 0])
    return t.done(eng)


def s2_trip_after_a_done_ticket():
    t = Trace(items=40, begin_rc=-5)  # (two passes stay below 100 items: the forward after them trips)
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    with t.call("forward_by_length_begin", via="forward_by_length"):
        t.tickets["done"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
        t.tickets["small"] = eng.forward_by_length_begin(IDS[:1], LENS[:1])  # (too small to be grouped: no library ticket either)
    t.stamp("form after begin", eng.form)
    via_forward(t, eng)
    with t.call("forward_by_length_end", via="forward_by_length"):
        t.stamp("end done", eng.forward_by_length_end(t.tickets["done"])["best"][0, 0])
        t.stamp("end small", eng.forward_by_length_end(t.tickets["small"])["best"][0, 0])
    return t.done(eng)


def s2_trip_in_a_kept_sweep():
    t = Trace(items=60, sink_share=1.0)
    eng = t.engine()
    with t.call("anchor_append 5"):
        eng.anchor_append(IDS[:5], LENS[:5])
    with t.call("bucketed_sweep keep topk", via="corpus_results"):
        best, idx, ps = eng.bucketed_sweep(IDS, RAGGED, 4, keep=True, topk=3)
        t.stamp("sweep", [best[:, 0].tolist(), idx.tolist()])
    with t.call("rematch_sweep"):
        t.stamp("rematch 1", eng.rematch_sweep()[1].tolist())
    with t.call("anchor_append 1"):
        eng.anchor_append(IDS[:1], LENS[:1])
    with t.call("rematch_sweep after append"):
        t.stamp("rematch 2", eng.rematch_sweep()[1].tolist())
    with t.call("rematch_sweep with_probs"):
        t.stamp("rematch 3", list(eng.rematch_sweep(with_probs=True)[2].shape))
    with t.call("sweep_topk"):
        p, i = eng.sweep_topk()
        t.stamp("sweep_topk", [list(p.shape), i[:, 0].tolist()])
    t.stamp("rematches", [list(c) for c in t.lib.log if c[0] == "rematch"])
    return t.done(eng)


def s2_trip_after_a_kept_sweep():
    """The stored results are the default form's, the bank is encoded again by a trip in anchor_append: g_first 0, then the covered count."""
    t = Trace(items=60, sink_share=0.0)
    eng = t.engine()
    with t.call("anchor_append 5"):
        eng.anchor_append(IDS[:5], LENS[:5])
    with t.call("bucketed_sweep keep"):
        eng.bucketed_sweep(IDS, RAGGED, 8, keep=True)
    t.lib.sink_share = 1.0
    with t.call("anchor_append 2"):
        eng.anchor_append(IDS[:2], LENS[:2])
    with t.call("rematch_sweep"):
        eng.rematch_sweep()
    with t.call("anchor_append 1"):
        eng.anchor_append(IDS[:1], LENS[:1])
    with t.call("rematch_sweep after append"):
        eng.rematch_sweep()
    t.stamp("rematches", [list(c) for c in t.lib.log if c[0] == "rematch"])
    return t.done(eng)


def s3_no_trip(safe_already=False, **lib_kw):
    t = Trace(**lib_kw)
    eng = t.engine()
    if safe_already:
        with t.call("set_form safe"):
            eng.set_form("safe")
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    via_forward(t, eng)
    via_anchor_append(t, eng)
    via_by_length_end(t, eng)
    via_bucketed_sweep(t, eng)
    return t.done(eng)


def s4_guarded_load(option=None, compute="guarded", handle_form=None):
    t = Trace(flag_share=0.0)
    if handle_form is not None:
        t.lib.form = handle_form  # (MEMVUL_FORM, read by mv_create)
    eng = t.engine()
    if option is not None:
        eng._sink_tokens_wanted = binding._sink_token_list(option)
    with t.call("load_state_dict"):
        eng.load_state_dict({"scalar": np.float32(1.0)}, compute)
    with t.call("sink_tokens"):
        t.stamp("sink_tokens", eng.sink_tokens())
    t.stamp("precise", bool(eng._precise))
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    via_forward(t, eng)
    via_encode(t, eng)
    with t.call("set_sink_tokens"):
        eng.set_sink_tokens([])
        t.stamp("cleared", eng.sink_tokens())
    return t.done(eng)


def s4_share_warning(flag_share):
    t = Trace(rows=200, flag_share=flag_share, route_share=0.5, items=1000, sink_share=1.0)
    eng = t.engine()
    with t.call("set_form + anchor_set + set_sink_tokens"):
        eng.set_form("guarded")
        eng.anchor_set(bank(2))
        eng.set_sink_tokens([1012])
    via_forward(t, eng)
    via_forward(t, eng)
    via_encode(t, eng)
    via_anchor_append(t, eng)
    via_by_length_end(t, eng)
    via_bucketed_sweep(t, eng)
    with t.call("the counters"):
        t.stamp("route_stats", [eng.route_stats(), eng.route_stats(reset=True), eng.route_stats()])
        t.stamp("form_stats", list(eng.form_stats()))
        t.stamp("last_row_forms", eng.last_row_forms())
        t.stamp("corpus_row_forms", eng.corpus_row_forms(2, 5))
    return t.done(eng)


def s4_share_warning_from(entry):
    t = Trace(rows=200, flag_share=0.26)
    eng = t.engine()
    with t.call("set_form + anchor_set"):
        eng.set_form("guarded")
        eng.anchor_set(bank(2))
    ENTRY_POINTS[entry](t, eng)
    return t.done(eng)


def s5_saturation(entry):
    t = Trace(saturated=7, sink_share=0.0)
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    ENTRY_POINTS[entry](t, eng)
    via_forward(t, eng)
    via_encode(t, eng)
    with t.call("x8_saturation"):
        t.stamp("x8_saturation", eng.x8_saturation())
    return t.done(eng)


def s6_errors():
    t = Trace(sink_share=0.0)
    eng = t.engine()
    with t.call("anchor_set"):
        eng.anchor_set(bank(2))
    with t.call("begin 1, 2"):
        t.tickets["t1"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
        t.tickets["t2"] = eng.forward_by_length_begin(IDS, LENS, min_tokens=256)
    with t.call("a ticket collected out of order"):
        eng.forward_by_length_end(t.tickets["t2"])
    with t.call("in order"):
        eng.forward_by_length_end(t.tickets["t1"])
        eng.forward_by_length_end(t.tickets["t2"])
    with t.call("rematch_sweep before any sweep"):
        eng.rematch_sweep()
    with t.call("sweep_topk before any sweep"):
        eng.sweep_topk()
    with t.call("bucketed_sweep topk alone"):
        eng.bucketed_sweep(IDS, RAGGED, 4, topk=2)
    with t.call("rematch_sweep without keep"):
        eng.rematch_sweep()
    with t.call("bucketed_sweep keep alone"):
        eng.bucketed_sweep(IDS, RAGGED, 4, keep=True)
    with t.call("sweep_topk without topk"):
        eng.sweep_topk()
    with t.call("an unknown form"):
        eng.set_form("guardd")
    with t.call("an unknown compute dtype"):
        eng.load_state_dict({}, "guardd")
    with t.call("an unknown compute dtype code"):
        binding.compute_dtype_of(5)
    for what, fn in (("anchor_set", eng.anchor_set), ("match", eng.match), ("topk", lambda u: eng.topk(u, 2))):
        with t.call(what + " with the wrong width"):
            fn(np.zeros((2, 768), np.float32))
        with t.call(what + " with one dimension"):
            fn(np.zeros((512,), np.float32))
    for text in ("1012, 1010", "", ",".join(str(i) for i in range(65))):
        with t.call("parse_sink_tokens %r" % text[:12]):
            binding.parse_sink_tokens(text)
    with t.call("set_sink_tokens with a float"):
        eng.set_sink_tokens([1.5])
    with t.call("set_sink_tokens with a bool"):
        eng.set_sink_tokens([True])
    return t.done(eng)


def s6_sink_tokens_outside_the_guarded_form(compute, option):
    t = Trace()
    eng = t.engine()
    if option:
        eng._sink_tokens_wanted = [5]
    with t.call("load_state_dict"):
        eng.load_state_dict({}, compute)
    return t.done(eng)


def s6_environment():
    """The strict parsers, each on a value it refuses and on one it takes."""
    t = Trace()
    for name, fn, good, bad in (("MEMVUL_ON_SINK", binding.on_sink_policy, "safe", "SAFE"), ("MEMVUL_SINK_CENSUS", binding.sink_census_policy, "1", "yes"),
                                ("MEMVUL_TOKENIZE", binding.tokenize_policy, "gpu-utf8", "cpu"), ("MEMVUL_SINK_TOKENS", binding.sink_tokens_policy, "7,8", "7;8")):
        for value in (None, good, bad):
            with environment({} if value is None else {name: value}), t.call("%s=%r" % (name, value)):
                t.stamp("%s=%r" % (name, value), repr(fn()))
    with t.call("tokenize option"):
        t.stamp("tokenize option", binding.tokenize_policy("gpu"))
    with t.call("tokenize option refused"):
        binding.tokenize_policy("GPU")
    with environment({"MEMVUL_ON_SINK": "maybe"}), t.call("Engine() under a malformed MEMVUL_ON_SINK"):
        binding.Engine(0)
    with t.call("Engine() with a malformed sink_tokens"):
        binding.Engine(0, sink_tokens=[True])
    t.stamp("abi", sorted(binding.ABI_SYMBOLS))
    return t.done()


ENTRIES_THAT_READ = ("forward", "encode", "anchor_append", "forward_by_length", "forward_by_length_small", "forward_by_length_end", "corpus_results", "bucketed_sweep")
SAFE = {"MEMVUL_ON_SINK": "safe"}
# name -> (environment, scenario, arguments)
SCENARIOS = {"1 default form": ({}, s1_default_form, {})}
SCENARIOS.update({"1 the sink warning from " + e: ({}, s1_warning_from, {"entry": e}) for e in ENTRIES_THAT_READ})
SCENARIOS.update({"2 trip in " + e: (SAFE, s2_trip_from, {"entry": e}) for e in ENTRIES_THAT_READ})
SCENARIOS.update({
    "2 trip in anchor_append, the bank replayed": (SAFE, s2_trip_in_anchor_append_replays_the_bank, {}),
    "2 trip with an empty installed bank": (SAFE, s2_trip_with_an_empty_installed_bank, {}),
    "2 trip with two tickets in flight": (SAFE, s2_trip_with_two_tickets_in_flight, {}),
    "2 trip inside a done ticket": (SAFE, s2_trip_inside_a_done_ticket, {}),
    "2 trip after a done ticket": (SAFE, s2_trip_after_a_done_ticket, {}),
    "2 trip in a kept sweep": (SAFE, s2_trip_in_a_kept_sweep, {}),
    "2 trip after a kept sweep": (SAFE, s2_trip_after_a_kept_sweep, {}),
    "3 no trip below 100 items": (SAFE, s3_no_trip, {"items": 19, "sink_share": 1.0}),  # (five passes: 95 items)
    "3 no trip at exactly 2 %": (SAFE, s3_no_trip, {"items": 1000, "sink_share": 0.02}),
    "3 no trip in the safe form": (SAFE, s3_no_trip, {"safe_already": True}),
    "4 guarded, the list from the constructor": ({"MEMVUL_SINK_TOKENS": "3,4"}, s4_guarded_load, {"option": [9, 1012]}),
    "4 guarded, the list from the environment": ({"MEMVUL_SINK_TOKENS": "1012,1010,1012"}, s4_guarded_load, {}),
    "4 guarded, no list": ({}, s4_guarded_load, {}),
    "4 guarded by the handle's form": ({"MEMVUL_SINK_TOKENS": "7"}, s4_guarded_load, {"compute": "precise", "handle_form": binding.MV_FORM_GUARDED}),
    "4 rescored share 0.26": ({}, s4_share_warning, {"flag_share": 0.26}),
    "4 rescored share 0.25": ({}, s4_share_warning, {"flag_share": 0.25}),
    "4 rescored share 0.26 under MEMVUL_ON_SINK=safe": (SAFE, s4_share_warning, {"flag_share": 0.26}),
})
SCENARIOS.update({"4 the share warning from " + e: ({}, s4_share_warning_from, {"entry": e}) for e in ENTRIES_THAT_READ})
SCENARIOS.update({"5 saturation from " + e: ({}, s5_saturation, {"entry": e}) for e in ENTRIES_THAT_READ})
SCENARIOS.update({
    "6 errors": ({}, s6_errors, {}),
    "6 the strict environment": ({}, s6_environment, {}),
})
SCENARIOS.update({"6 a sink-token list on %s (%s)" % (c, "option" if o else "environment"):
                  ({} if o else {"MEMVUL_SINK_TOKENS": "1012"}, s6_sink_tokens_outside_the_guarded_form, {"compute": c, "option": o})
                  for c in ("precise", "safe", "f16") for o in (False, True)})


def run(name) -> dict:
    env, scenario, kw = SCENARIOS[name]
    with environment(env):
        return scenario(**kw)


def run_all() -> dict:
    return {name: run(name) for name in SCENARIOS}
