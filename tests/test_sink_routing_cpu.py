"""The sink-token list of the guarded form (include/memvul_hip.h mv_set_sink_tokens), the parts that need no GPU: the ABI in all three places, the routing rule
(mv_route_scan, host only) against a numpy restatement, the host logic of binding.Engine against a stand-in library, and the audit's plumbing."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest

from memvul_amd import audit, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_f32_form_cpu as f32cpu  # noqa: E402  (the oracle-backed audit stand-in)
import test_guarded_form_cpu as gf  # noqa: E402  (the recorder library of the guarded form)
import test_safe_form_cpu as sf  # noqa: E402

MV_ERR_INVALID = -1
NEW = ("mv_set_sink_tokens", "mv_get_sink_tokens", "mv_route_stats", "mv_route_scan", "mv_corpus_route_flags")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_carry_the_sink_token_list():
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    from stage_kit import host_source

    src = host_source()
    lib = binding.load_library()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in binding.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\nint %s\([^)]*\) try \{" % name, src), name  # every int mv_* is a function-try-block
        assert getattr(lib, name).restype == C.c_int
    i32p, i64p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p
    assert lib.mv_set_sink_tokens.argtypes == [vp, i32p, C.c_int]
    assert lib.mv_get_sink_tokens.argtypes == [vp, i32p, C.c_int]
    assert lib.mv_route_stats.argtypes == [vp, i64p, C.c_int]
    assert lib.mv_route_scan.argtypes == [vp, vp, C.c_int, C.c_int, i32p, C.c_int, C.c_int, vp]
    assert lib.mv_corpus_route_flags.argtypes == [vp, C.c_int64, C.c_int64, vp]
    assert re.search(r"#define MV_MAX_SINK_TOKENS 64\b", hdr) and binding.MAX_SINK_TOKENS == 64
    # no new form constant, no new library environment switch: MEMVUL_SINK_TOKENS is the Python surface's
    env = hdr[hdr.index("Environment switches read HERE"):]
    assert "six" in env[:200] and "MEMVUL_SINK_TOKENS" in hdr and "MEMVUL_SINK_TOKENS" not in src
    assert len(re.findall(r"#define MV_FORM_\w+", hdr)) == 3
    assert "route.h" in open(os.path.join(ROOT, "memvul_amd", "build.py")).read()
    for fn in ("set_sink_tokens", "sink_tokens", "route_stats", "route_scan", "corpus_route_flags"):
        assert hasattr(binding.Engine, fn), fn


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------------------------

B = 70
LENGTHS = {64: (1, 2, 3, 15, 16, 17, 63, 64), 512: (1, 2, 3, 15, 16, 17, 63, 64, 257, 511, 512)}
PLACEMENTS = ("pos0", "last", "at1", "len-2", "at_len", "S-1", "twice", "absent")


def rule(ids, lens, tokens):
    """The routing rule restated: a row is routed iff a token at positions 1 .. len - 2 is in the list."""
    pos = np.arange(ids.shape[1])[None, :]
    window = (pos >= 1) & (pos < np.asarray(lens)[:, None] - 1)
    return (np.isin(ids, np.asarray(tokens, np.int64)) & window).any(1)


def token_lists(vocab):
    """Lists of 1, 2 and 64 ids, with duplicates, with id 0 (the padding id) and id vocab - 1."""
    many = [0, vocab - 1] + [11 + 29 * i for i in range(40)] + [11 + 29 * i for i in range(22)]  # 64 ids, 22 of them twice
    assert len(many) == 64 and max(many) < vocab
    return {"one": [vocab - 1], "one_mid": [vocab // 2], "two_with_zero": [0, 1012 % vocab], "two_same": [77, 77], "many": many}


def matrix(S, vocab, tokens, shift):
    """70 rows over the (length, placement) pairs of width S, starting `shift` pairs in (at S = 512 there are 88 pairs: the matrices of one width cover them
    between them), 0-padded; the base ids avoid the list and 0."""
    pairs = list(itertools.product(LENGTHS[S], PLACEMENTS))
    rng = np.random.default_rng(1000 * S + vocab + shift)
    allowed = np.setdiff1d(np.arange(1, vocab), np.asarray(tokens))
    ids = np.zeros((B, S), np.int32)
    lens = np.zeros(B, np.int32)
    used = set()
    for b in range(B):
        n, where = pairs[(shift + b) % len(pairs)]
        used.add((n, where))
        ids[b, :n] = rng.choice(allowed, n)
        lens[b] = n
        t = tokens[b % len(tokens)]
        spots = {"pos0": [0], "last": [n - 1], "at1": [1], "len-2": [n - 2], "at_len": [n], "S-1": [S - 1], "twice": [1, n - 2], "absent": []}[where]
        for p in spots:
            if 0 <= p < S:
                ids[b, p] = t
    return ids, lens, used


def cases():
    for S in (64, 512):
        seen = set()
        for vocab in (2048, 30522):
            for k, (name, tokens) in enumerate(token_lists(vocab).items()):
                ids, lens, used = matrix(S, vocab, tokens, shift=17 * k + (35 if vocab == 2048 else 0))
                seen |= used
                yield S, vocab, name, tokens, ids, lens
        assert seen == set(itertools.product(LENGTHS[S], PLACEMENTS)), S  # every (length, placement) pair was in some matrix of this width


def test_route_scan_is_the_rule():
    n_cases = routed_total = 0
    for S, vocab, name, tokens, ids, lens in cases():
        want = rule(ids, lens, tokens)
        got = binding.Engine.route_scan(ids, lens, tokens, vocab_size=vocab)
        assert got.dtype == bool and np.array_equal(got, want), (S, vocab, name, np.flatnonzero(got != want))
        # what the placements mean, independent of the restatement: nothing of 1 or 2 tokens is ever routed, and padding (id 0 in the list) routes nothing
        assert not got[lens <= 2].any()
        if 0 in tokens:
            clean = ids.copy()  # every listed id taken out of the real tokens; the padding keeps its zeros
            clean[np.isin(clean, tokens) & (np.arange(S)[None, :] < lens[:, None])] = 5
            assert not binding.Engine.route_scan(clean, lens, tokens, vocab_size=vocab).any(), (S, vocab, name)
        n_cases += 1
        routed_total += int(got.sum())
        assert 0 < got.sum() < B, (S, vocab, name, int(got.sum()))
    assert n_cases == 20 and routed_total > 0
    # an empty list routes nothing; id vocab - 1 at a routed position routes
    ids, lens, _ = matrix(64, 2048, [2047], 0)
    assert not binding.Engine.route_scan(ids, lens, [], vocab_size=2048).any()
    row = np.array([[5, 2047, 6, 0]], np.int32)
    assert binding.Engine.route_scan(row, np.array([3], np.int32), [2047], vocab_size=2048).tolist() == [True]
    assert binding.Engine.route_scan(row, np.array([2], np.int32), [2047], vocab_size=2048).tolist() == [False]


def test_route_scan_error_paths_leave_the_flags_alone():
    lib = binding.load_library()
    ids, lens, _ = matrix(64, 2048, [9], 0)
    good = (C.c_int32 * 2)(9, 10)

    def call(ids_=ids, lens_=lens, B_=B, S_=64, tokens=good, n=2, vocab=2048, with_flags=True):
        flags = np.full(B, 7, np.uint8)
        rc = lib.mv_route_scan(binding._ptr(ids_), binding._ptr(lens_), B_, S_, tokens, n, vocab, binding._ptr(flags) if with_flags else None)
        assert (flags == 7).all() or rc == 0
        return rc

    assert call() == 0
    assert call(n=0, tokens=None) == 0  # an empty list is no error (tokens may be NULL then)
    assert call(n=-1) == MV_ERR_INVALID
    assert call(n=65, tokens=(C.c_int32 * 65)(*range(65))) == MV_ERR_INVALID
    assert call(n=2, tokens=None) == MV_ERR_INVALID
    assert call(tokens=(C.c_int32 * 2)(9, 2048)) == MV_ERR_INVALID  # outside [0, vocab)
    assert call(tokens=(C.c_int32 * 2)(-1, 9)) == MV_ERR_INVALID
    assert call(ids_=None) == MV_ERR_INVALID and call(lens_=None) == MV_ERR_INVALID and call(with_flags=False) == MV_ERR_INVALID
    assert call(S_=0) == MV_ERR_INVALID and call(B_=-1) == MV_ERR_INVALID and call(vocab=0) == MV_ERR_INVALID
    assert call(n=64, tokens=(C.c_int32 * 64)(*range(64))) == 0
    with pytest.raises(RuntimeError, match="mv_route_scan"):
        binding.Engine.route_scan(ids, lens, [2048], vocab_size=2048)
    with pytest.raises(ValueError):
        binding.Engine.route_scan(ids, lens, [1.5], vocab_size=2048)


def test_the_guarded_fixture_is_split_by_the_rule(golden_dir):
    """On the three mixed cases of the guarded suite the list [MID_ID] selects exactly the marked reports and anchors and no clean row."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_guarded_form_refs as mg
    from memvul_amd import synth

    refs = np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))
    for case in ("mid_all_80_3001", "mid_all_50_3002", "mid_cls_80_3003"):
        dims, _, ids, lens, aids, alens, marked, amarked = mg.mixed_case(case, refs)
        assert marked.tolist() == list(range(8)) and amarked.tolist() == list(range(6))
        assert np.flatnonzero(binding.Engine.route_scan(ids, lens, [synth.MID_ID], vocab_size=dims.vocab_size)).tolist() == marked.tolist()
        assert np.flatnonzero(binding.Engine.route_scan(aids, alens, [synth.MID_ID], vocab_size=dims.vocab_size)).tolist() == amarked.tolist()
        assert not (mg.unmark(ids) == synth.MID_ID).any()


# ---- the host logic of binding.Engine ---------------------------------------------------------------------------------------------------------------------------

class _Quick(gf._Quick):
    pass


class _Lib(gf._Lib):
    """The guarded form's recorder + the list: finalize, set / get, and a route counter fed by every pass-like call in the guarded form."""

    def __init__(self, route_share=0.25, **kw):
        super().__init__(**kw)
        self.tokens, self.routed, self.route_share = [], 0, route_share

    def _pass(self):
        super()._pass()
        if self.form == binding.MV_FORM_GUARDED and self.tokens:
            self.routed += int(self.rows * self.route_share)

    def mv_finalize_weights(self, h, code):
        self.log.append(("finalize", code))
        return 0

    def mv_set_sink_tokens(self, h, ids, n):
        self.log.append(("set_sink_tokens", [int(ids[i]) for i in range(n)]))
        self.tokens = [int(ids[i]) for i in range(n)]
        return 0

    def mv_get_sink_tokens(self, h, ids, cap):
        for i, t in enumerate(self.tokens[:cap]):
            ids[i] = t
        return len(self.tokens)

    def mv_route_stats(self, h, n, reset):
        self.log.append(("route_stats", int(reset)))
        n._obj.value = self.routed
        if reset:
            self.routed = 0
        return 0


def test_the_environment_value_is_parsed_strictly(monkeypatch):
    assert binding.parse_sink_tokens("1012,1010") == [1012, 1010] and binding.parse_sink_tokens("7") == [7] and binding.parse_sink_tokens("5,5") == [5, 5]
    for bad in ("", ",", "1012,", ",1", "1 ,2", " 1", "1,,2", "a", "-1", "+1", "0x10", "1012;1010", "1.0", "1,2\n"):
        with pytest.raises(ValueError, match="MEMVUL_SINK_TOKENS"):
            binding.parse_sink_tokens(bad)
    with pytest.raises(ValueError, match="at most 64"):
        binding.parse_sink_tokens(",".join(str(i) for i in range(65)))
    monkeypatch.delenv("MEMVUL_SINK_TOKENS", raising=False)
    assert binding.sink_tokens_policy() is None
    monkeypatch.setenv("MEMVUL_SINK_TOKENS", "3,4")
    assert binding.sink_tokens_policy() == [3, 4]
    monkeypatch.setenv("MEMVUL_SINK_TOKENS", "3, 4")
    with pytest.raises(ValueError, match="MEMVUL_SINK_TOKENS"):
        binding.Engine(0)  # (before anything is created or loaded)


@pytest.mark.parametrize("compute", ["precise", "safe", "f16"])
def test_the_switch_is_refused_outside_the_guarded_form(monkeypatch, compute):
    monkeypatch.setenv("MEMVUL_SINK_TOKENS", "1012")
    lib = _Lib()
    eng = sf.StandInEngine(lib)
    with pytest.raises(ValueError, match="guarded form only"):
        eng.load_state_dict({}, compute)
    assert not [c for c in lib.log if c[0] == "set_sink_tokens"]
    # the option of engine_options says so under its own name
    monkeypatch.delenv("MEMVUL_SINK_TOKENS")
    eng = sf.StandInEngine(_Lib())
    eng._sink_tokens_wanted = [5]
    with pytest.raises(ValueError, match="sink_tokens is set"):
        eng.load_state_dict({}, compute)


def test_the_list_is_applied_once_after_finalize(monkeypatch):
    monkeypatch.setenv("MEMVUL_SINK_TOKENS", "1012,1010,1012")
    lib = _Lib(flag_share=0.0)
    eng = sf.StandInEngine(lib)
    eng.load_state_dict({}, "guarded")
    assert [c[0] for c in lib.log] == ["finalize", "set_form", "set_sink_tokens"] and lib.log[-1][1] == [1012, 1010, 1012]
    assert eng.sink_tokens() == [1012, 1010, 1012]
    eng.anchor_set(np.zeros((2, 512), np.float32))
    eng.forward(sf.IDS, sf.LENS)
    eng.encode(sf.IDS, sf.LENS)
    assert len([c for c in lib.log if c[0] == "set_sink_tokens"]) == 1
    # MEMVUL_FORM=guarded (read by mv_create) with the default compute dtype: the form the handle reports decides
    lib = _Lib()
    lib.form = binding.MV_FORM_GUARDED
    eng = sf.StandInEngine(lib)
    eng.load_state_dict({}, "precise")
    assert eng.form == "guarded" and lib.tokens == [1012, 1010, 1012]
    # the option wins over the environment; an empty option clears
    lib = _Lib()
    eng = sf.StandInEngine(lib)
    eng._sink_tokens_wanted = [9]
    eng.load_state_dict({}, "guarded")
    assert lib.tokens == [9]
    # nothing set: nothing called
    monkeypatch.delenv("MEMVUL_SINK_TOKENS")
    lib = _Lib()
    sf.StandInEngine(lib).load_state_dict({}, "guarded")
    assert not [c for c in lib.log if c[0] == "set_sink_tokens"]
    with pytest.raises(ValueError, match="integer token ids"):
        eng.set_sink_tokens([1.5])
    with pytest.raises(ValueError, match="integer token ids"):
        binding.Engine(0, sink_tokens=[True])


def test_route_stats_and_the_share_warning(monkeypatch):
    monkeypatch.delenv("MEMVUL_SINK_TOKENS", raising=False)
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    import warnings

    lib = _Lib(rows=200, flag_share=0.26, route_share=0.5)
    eng = gf._guarded_engine(lib)
    eng.set_sink_tokens([1012])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.forward(sf.IDS, sf.LENS)
        eng.forward(sf.IDS, sf.LENS)
    assert eng.route_stats() == 200 and eng.route_stats(reset=True) == 200 and eng.route_stats() == 0
    assert [c for c in lib.log if c[0] == "route_stats"] == [("route_stats", 0), ("route_stats", 1), ("route_stats", 0)]
    assert eng.form_stats() == (400, 104)  # mv_form_stats keeps its meaning: the routed sequences are not in it
    # the one warning keeps its rule on the RESCORED share and now points at the census and the list
    told = sf._told(rec, "guarded form")
    assert len(told) == 1 and "52 of 200" in told[0] and "sink_census" in told[0] and "MEMVUL_SINK_TOKENS" in told[0]
    lib = _Lib(rows=200, flag_share=0.0, route_share=1.0)  # everything routed, nothing rescored: no warning
    eng = gf._guarded_engine(lib)
    eng.set_sink_tokens([1012])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.forward(sf.IDS, sf.LENS)
    assert not rec and eng.route_stats() == 200


# ---- the audit ------------------------------------------------------------------------------------------------------------------------------------------------

class _AuditStandin(f32cpu._Standin):
    lists = []

    def set_sink_tokens(self, ids):
        _AuditStandin.lists.append((self.compute, list(ids)))
        self.tokens = list(ids)

    def form_stats(self):
        return 40, 4

    def route_stats(self):
        return 10 if getattr(self, "tokens", None) else 0


def test_audit_hands_the_list_to_the_guarded_form_alone(small_case=None):
    from memvul_amd import synth

    dims = synth.BertDims(layers=2)
    w = synth.make_weights(dims, qk_scale=2.0, match_scale=6.0)
    ids, lens = synth.make_ids(6, 48, dims.vocab_size, seed=5, ragged=True, min_len=8)
    aids, alens = synth.make_ids(3, 70, dims.vocab_size, seed=6, ragged=True, min_len=10)
    f32cpu._Standin.created, f32cpu._Standin.marks, _AuditStandin.lists = [], (), []
    res = audit.audit(w, ids, lens, aids, alens, forms=("precise", "guarded"), engine_factory=_AuditStandin, sink_tokens=[1012, 1010])
    assert _AuditStandin.lists == [("guarded", [1012, 1010])]
    g = res["forms"]["guarded"]
    assert g["sink_token_list"] == [1012, 1010] and g["routed_share"] == pytest.approx(0.25) and g["rescored_share"] == pytest.approx(0.1)
    assert g["monitors"]["guarded_routed"] == 10 and "routed_share" not in res["forms"]["precise"]
    json.dumps(res)
    # without the list the object is what it was
    res = audit.audit(w, ids, lens, aids, alens, forms=("guarded",), engine_factory=_AuditStandin)
    assert "routed_share" not in res["forms"]["guarded"] and "guarded_routed" not in res["forms"]["guarded"]["monitors"]
    assert _AuditStandin.lists == [("guarded", [1012, 1010])]
    with pytest.raises(ValueError, match="guarded"):
        audit.audit(w, ids, lens, aids, alens, forms=("precise", "safe"), engine_factory=_AuditStandin, sink_tokens=[1012])
    with pytest.raises(ValueError):
        audit.audit(w, ids, lens, aids, alens, forms=("guarded",), engine_factory=_AuditStandin, sink_tokens=[1.5])


def test_the_command_line_takes_the_list_and_refuses_it_without_guarded(capsys, monkeypatch):
    import plumbing_util as pu
    import shutil

    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=6, n_anchors=3, layers=2)
    try:
        monkeypatch.chdir(root)
        f32cpu._Standin.created, f32cpu._Standin.marks, _AuditStandin.lists = [], (), []
        base = ["--archive", arch, "--golden", golden, "--input", test_path]
        rc = audit.main(base + ["--forms", "precise,guarded", "--sink-tokens", "12,10"], engine_factory=_AuditStandin)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert rc == 0 and len(lines) == 1
        res = json.loads(lines[0])
        assert res["forms"]["guarded"]["routed_share"] == pytest.approx(0.25) and res["forms"]["guarded"]["sink_token_list"] == [12, 10]
        assert _AuditStandin.lists == [("guarded", [12, 10])]
        for bad in (["--forms", "precise", "--sink-tokens", "12"], ["--sink-tokens", "12"], ["--forms", "guarded", "--sink-tokens", "12, 10"],
                    ["--forms", "guarded", "--sink-tokens", ""]):
            with pytest.raises(SystemExit) as e:
                audit.main(base + bad, engine_factory=_AuditStandin)
            assert e.value.code == 2
            assert "sink-tokens" in capsys.readouterr().err
        assert _AuditStandin.lists == [("guarded", [12, 10])]
    finally:
        shutil.rmtree(root, ignore_errors=True)
