"""The sink census (memvul_amd/csrc/sink_census.h; include/memvul_hip.h mv_sink_census_enable / mv_sink_census_read) against a float64 reference, on the GPU.

Reference: tests/golden/sink_census_refs.npz (scripts/make_sink_census_refs.py describes the models, the lengths and the sink positions): per (layer, sequence,
head) item the exact collision mass of the [CLS] row on the ordinary keys, the position of the largest ordinary share, that share, the runner-up and the third
share.  An item is UNCERTAIN when its collision mass lies inside the monitor suite's band around 0.25 (delta_abs of tests/golden/monitor_refs.npz = 4.2e-3, plus
2^-10 x the mass) or when its two largest shares belong to different tokens and are closer than m = 3 x the largest |rounding-model p - exact p| of the fixture
(stored in the npz; no GPU value enters it).  tests/census_kit.py check_census holds the checks: per token lo <= items <= hi, tokens outside both exactly 0,
by_head bounded likewise with the same total, the total inside the interval the monitor's own items_over is allowed, the mean share within m of the reference's
(plus what uncertain items could add).

At padded width 192 the default form's GEMMs take their form from the WHOLE pass (tests/test_monitor_parity_gpu.py's docstring): where single rows are compared
bit for bit with their batch — every batch of the fixture holds rows of fewer than 128 tokens — a row travels with a 15-token companion, which the census skips.

Every test records what it measured (gu.record "sink_census_*")."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import census_kit as ck  # noqa: E402
import make_sink_census_refs as mk  # noqa: E402
from memvul_amd import synth  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402

COMPUTE = {"default": "precise", "safe": "safe", "guarded": "guarded"}
V = mk.DIMS["vocab_size"]
SWITCHES = ("MEMVUL_CLS_PRUNE", "MEMVUL_STREAMS", "MEMVUL_QKV_ASIDE", "MEMVUL_CLS_ASIDE", "MEMVUL_CLS_ASIDE_MIN_LEN", "MEMVUL_FORM", "MEMVUL_SINK_CENSUS", "MEMVUL_ON_SINK")
MV_ERR_INVALID, MV_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def refs(golden_dir):
    r = np.load(os.path.join(golden_dir, "sink_census_refs.npz"))
    return {k: r[k] for k in r.files}


@pytest.fixture(scope="module")
def delta_abs(golden_dir):
    return float(np.load(os.path.join(golden_dir, "monitor_refs.npz"))["delta_abs"])


_engines, _weights = {}, {}


def _w(refs, model):
    if model not in _weights:
        _weights[model] = mk.weights(model, refs[model + "_gains"])
    return _weights[model]


def _engine(refs, model, compute="precise", prune=True, census=True):
    """A cached engine of one fixture model (two alive at most), the census on unless asked otherwise."""
    key = (model, compute, prune, census)
    if key not in _engines:
        while len(_engines) >= 2:
            _engines.pop(next(iter(_engines))).close()
        old = {k: os.environ.pop(k, None) for k in SWITCHES}
        if not prune:
            os.environ["MEMVUL_CLS_PRUNE"] = "0"
        try:
            e = Engine(0, vocab_size=V, layers=mk.DIMS["layers"], max_tokens=16384, max_batch=64, max_anchors=64)
        finally:
            os.environ.pop("MEMVUL_CLS_PRUNE", None)
            os.environ.update({k: v for k, v in old.items() if v is not None})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            e.load_state_dict(_w(refs, model), compute)
        if census:
            e.sink_census_enable(True)
        _engines[key] = e
    return _engines[key]


def _quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the default form warns once about the sink it sees)
        return f(*a, **k)


def _census_of(eng, call):
    eng.sink_census_read(reset=True)
    _quiet(call)
    return eng.sink_census_read()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _add(hists):
    hists = list(hists)
    return tuple(sum(h[i].astype(np.uint64) for h in hists).astype(hists[0][i].dtype) for i in range(3))


_COMPANION = {}


def _companion(W):
    if W not in _COMPANION:
        ids, _ = synth.make_ids(1, W, V, seed=77)
        ids[0, 14], ids[0, 15:] = synth.SEP_ID, 0
        _COMPANION[W] = ids
    return _COMPANION[W]


def _row_alone(eng, ids_row, n, W, ragged_pass):
    """The census of ONE sequence encoded at width W; ragged_pass: in the pass form of a batch whose shortest row is below 128 tokens (module docstring)."""
    ids, lens = ids_row[None, :W], np.array([n], np.int32)
    if ragged_pass and ck.MIN_LEN <= n and W > 128 and (-(-W // 64) * 64 if W <= 256 else -(-W // 128) * 128) in (192, 384):
        ids, lens = np.concatenate([ids, _companion(W)]), np.array([n, 15], np.int32)
    return _census_of(eng, lambda: eng.encode(np.ascontiguousarray(ids, np.int32), lens))


def _padded(n):
    return -(-n // 64) * 64 if n <= 256 else -(-n // 128) * 128


# ---- a. the histogram against the reference --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("form", ["default", "safe"])
@pytest.mark.parametrize("model", list(mk.MODELS))
def test_the_histogram_lies_inside_what_the_reference_allows(gu, refs, delta_abs, model, form, prune):
    """a. Every (model, width) case as one batch of 8 through encode: check_census against the case's bounds over the monitored layers (2 pruned, 3 with
    MEMVUL_CLS_PRUNE=0); the two controls read all-zero histograms; the census total lies where the monitor's own items_over of the same call may lie, and the
    monitor's reading of that call is inside the same interval."""
    eng = _engine(refs, model, COMPUTE[form], prune)
    assert eng.form == form
    layers = mk.DIMS["layers"] - (1 if prune else 0)
    m, control = float(refs["m"]), mk.MODELS[model][4]
    bad, gaps, totals = [], {}, {}
    for W in mk.WIDTHS:
        ids, lens, _ = mk.case_inputs(model, W)
        bd = ck.bounds(mk.case_ref(refs, model, W), ids, lens, layers, V, delta_abs, m)
        eng.attention_concentration(reset=True)
        got = _census_of(eng, lambda: eng.encode(ids, lens))
        _, over, total = eng.attention_concentration()
        what = f"{model}, {form} form, {'pruned' if prune else 'MEMVUL_CLS_PRUNE=0'}, width {W}"
        b, gaps[W] = ck.check_census(got, bd, m, what, controls=control)
        bad += b
        assert got[2][layers:].sum() == 0, what  # (no layer that feeds no monitor)
        assert total == 12 * layers * int((lens >= ck.MIN_LEN).sum()), (what, total)
        if not int(bd["head_lo"].sum()) <= over <= int(bd["head_hi"].sum()):
            bad.append(f"{what}: the monitor's items_over {over} outside [{int(bd['head_lo'].sum())}, {int(bd['head_hi'].sum())}]")
        totals[W] = (int(got[0].sum()), int(over))
    print(f"{model} {form} prune={prune}: largest |GPU mean share - exact| per width {gaps}; (census items, monitor items_over) per width {totals}")
    gu.record("sink_census_rows", model=model, form=form, prune=prune, m=m, **{"gap_%d" % W: g for W, g in gaps.items()},
              **{"items_%d" % W: t[0] for W, t in totals.items()}, **{"monitor_over_%d" % W: t[1] for W, t in totals.items()})
    assert not bad, "\n".join(bad)


# ---- b. integers: batches, entry points, streams, order ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", mk.WIDTHS)
def test_a_batch_reads_the_sum_of_its_rows_through_every_entry_point(gu, refs, W):
    """b. The histogram of a batch is bit-equal to the sum of its rows run one by one (width 192: in the batch's pass form), and bit-equal through encode,
    anchor_append, forward, a permutation of the batch and the resident sweep on one and on two streams; forward_by_length and two tickets in flight read the
    sum of the rows alone at the padded length of their own token count."""
    model = "two_tok"
    eng = _engine(refs, model)
    assert eng.form == "default"
    ids, lens, _ = mk.case_inputs(model, W)
    B = len(lens)
    at_w = _add(_row_alone(eng, ids[i], int(lens[i]), W, True) for i in range(B))
    own = _add(_row_alone(eng, ids[i], int(lens[i]), min(W, _padded(int(lens[i]))), False) for i in range(B))
    assert at_w[0].sum() > 0
    perm = np.random.Generator(np.random.PCG64(W)).permutation(B)
    seen = {}

    def through(name, call, want, times=1):
        got = seen[name] = _census_of(eng, call)
        assert _same(got, tuple(times * x for x in want)), (name, int(got[0].sum()), times * int(want[0].sum()), np.flatnonzero(got[0]).tolist())

    try:
        eng.anchor_reset()
        through("encode", lambda: eng.encode(ids, lens), at_w)
        through("permuted", lambda: eng.encode(np.ascontiguousarray(ids[perm]), lens[perm]), at_w)
        through("anchor_append", lambda: eng.anchor_append(ids, lens), at_w)
        through("forward", lambda: eng.forward(ids, lens), at_w)
        through("forward_by_length", lambda: eng.forward_by_length(ids, lens, min_tokens=1), own)

        def tickets():
            t = [eng.forward_by_length_begin(ids, lens, min_tokens=1) for _ in range(2)]
            assert all(x[0] == "pending" for x in t)
            for x in t:
                eng.forward_by_length_end(x)

        through("two tickets in flight", tickets, own, times=2)
        eng.corpus_upload(ids, lens)
        for streams in (1, 2):
            eng.set_streams(streams)
            through("corpus_run, %d stream(s)" % streams, lambda: (eng.corpus_run(0, B, 4), eng.corpus_results(0, B)), at_w)
    finally:
        eng.set_streams(2)
        eng.anchor_reset()
    gu.record("sink_census_entry_points", W=W, items=int(at_w[0].sum()), items_by_length=int(own[0].sum()), tokens=np.flatnonzero(at_w[0]).tolist())


def test_the_guarded_form_counts_every_sequence_once(gu, refs):
    """The rescoring passes of the guarded form run with the monitor detached and add nothing: a guarded engine's census equals the default form's on the same
    input — and rows WERE rescored."""
    out = {}
    for W in (192, 256):
        ids, lens, _ = mk.case_inputs("ord_80", W)
        d = _engine(refs, "ord_80", "precise")
        g = _engine(refs, "ord_80", "guarded")
        assert g.form == "guarded"
        want = _census_of(d, lambda: d.encode(ids, lens))
        g.form_stats(reset=True)
        got = _census_of(g, lambda: g.encode(ids, lens))
        out[W] = (int(got[0].sum()), g.form_stats()[1])
        assert _same(got, want) and want[0].sum() > 0 and g.form_stats()[1] > 0, (W, out)
    gu.record("sink_census_guarded", **{"items_rescored_%d" % W: list(v) for W, v in out.items()})


# ---- c. the ABI's edges ------------------------------------------------------------------------------------------------------------------------------------------

def test_reset_and_the_error_returns(refs):
    """reset zeroes everything; a read before the first enable is MV_ERR_STATE; a wrong vocab or head count is MV_ERR_INVALID; either pointer may be NULL;
    enabling on an f16 or an f32 engine is MV_ERR_STATE."""
    ids, lens, _ = mk.case_inputs("ord_80", 64)
    off = _engine(refs, "ord_80", census=False)
    lib, h = off._lib, off._h
    items = np.zeros(V, np.uint32)
    assert lib.mv_sink_census_read(h, items.ctypes.data, None, V, None, 36, 0) == MV_ERR_STATE
    eng = _engine(refs, "ord_80")
    got = _census_of(eng, lambda: eng.encode(ids, lens))
    assert got[0].sum() > 0
    again = eng.sink_census_read(reset=True)
    assert _same(got, again)
    assert not any(a.any() for a in eng.sink_census_read())
    lib, h = eng._lib, eng._h
    assert lib.mv_sink_census_read(h, items.ctypes.data, None, V + 1, None, 36, 0) == MV_ERR_INVALID
    assert lib.mv_sink_census_read(h, items.ctypes.data, None, V, None, 24, 0) == MV_ERR_INVALID
    assert lib.mv_sink_census_read(h, None, None, V, None, 36, 0) == 0
    for compute in ("f16", "f32"):
        e = _engine(refs, "ord_80", compute, census=False)
        assert e._lib.mv_sink_census_enable(e._h, 1) == MV_ERR_STATE
        with pytest.raises(RuntimeError):
            e.sink_census_enable(True)


def test_the_census_changes_nothing_else(refs):
    """With the census enabled, logits, best_idx and the three monitor counters are byte-equal to the same calls with it disabled."""
    ids, lens, _ = mk.case_inputs("two_tok", 192)
    res = {}
    for census in (False, True):
        eng = _engine(refs, "two_tok", census=census)
        try:
            eng.anchor_reset()
            eng.attention_concentration(reset=True)
            _quiet(eng.anchor_append, ids[:3], lens[:3])
            out = _quiet(eng.forward, ids, lens)
            out2 = _quiet(eng.forward_by_length, ids, lens, min_tokens=1)
            res[census] = (out["logits"].tobytes(), out["best_idx"].tobytes(), out2["logits"].tobytes(), np.float32(eng.attention_concentration()[0]).tobytes(),
                           eng.attention_concentration()[1:])
        finally:
            eng.anchor_reset()
    assert res[False] == res[True]


# ---- d. the Python surface ---------------------------------------------------------------------------------------------------------------------------------------

def test_sink_census_names_the_planted_token_first(gu, refs):
    eng = _engine(refs, "two_tok")
    ids, lens, _ = mk.case_inputs("two_tok", 256)
    vocab = {t: mk.VOCAB_WORDS.get(t, "tok%d" % t) for t in range(V)}
    eng.sink_census_read(reset=True)
    _quiet(eng.encode, ids, lens)
    c = eng.sink_census(top=5, vocab=vocab)
    rows = c["tokens"]
    assert rows[0]["token_id"] == synth.MID_ID and rows[0]["token"] == "." and rows[0]["items"] > 0 and 0.4 < rows[0]["mean_share"] <= 1.0, rows
    assert [r["token_id"] for r in rows[:2]] == [synth.MID_ID, mk.SECOND_ID] and rows[1]["token"] == "##ing", rows
    assert abs(sum(r["share_of_flagged_items"] for r in eng.sink_census(top=V)["tokens"]) - 1.0) < 1e-9
    assert c["by_head"].shape == (3, 12) and int(c["by_head"].sum()) == c["flagged_items"]
    assert "token" not in eng.sink_census(top=1)["tokens"][0]
    assert eng.sink_census(top=1, reset=True)["flagged_items"] > 0 and eng.sink_census()["tokens"] == []
    gu.record("sink_census_surface", rows=[{k: v for k, v in r.items()} for r in rows])


def test_the_audit_line_carries_sink_tokens_only_with_census(refs):
    from memvul_amd import audit

    ids, lens, _ = mk.case_inputs("ord_80", 256)
    opts = dict(max_tokens=16 * 512, max_batch=16, max_anchors=16)
    w = _w(refs, "ord_80")
    lines = {}
    for census in (False, True):
        res = audit.audit(w, ids, lens, ids[:2], lens[:2], forms=("precise", "f16"), engine_options=opts, census=census)
        res["reference"].pop("reports_per_s")
        for r in res["forms"].values():
            r.pop("reports_per_s")
        lines[census] = res
    st = lines[True]["forms"]["precise"].pop("sink_tokens")
    assert "sink_tokens" not in lines[True]["forms"]["f16"]
    assert json.dumps(lines[True]) == json.dumps(lines[False]) and "sink_tokens" not in json.dumps(lines[False])
    assert st[0]["token_id"] == synth.MID_ID and st[0]["items"] > 0
    holds = float(np.mean([(ids[b, :lens[b]] == synth.MID_ID).any() for b in range(len(lens))]))
    assert st[0]["sequences_with_token"] == holds
    json.dumps(st)
