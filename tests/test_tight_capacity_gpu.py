"""The guarded form and the sink-token list on an engine too small for the batch, on the GPU.

Every guarded or routed batch of tests/test_guarded_form_gpu.py and tests/test_sink_routing_gpu.py fits one pass per width and one upload / download per call
(max_tokens = 16 * 512, max_batch = 16, 16 rows).  Here the same kind of batch runs on that roomy engine and on a tight one (max_tokens = 4 * 256, max_batch = 8:
a pass holds 4 rows at 256 tokens, 8 at 128 and at 64), where
  * forward / encode at S = 256 run four passes with one upload and one download each, and their rescoring plan of the 8 marked rows has two passes,
  * the by-length group of six 256-token rows is cut 4 + 2,
  * a sweep of the whole corpus at 256 tokens leaves more flagged rows at one width than one rescoring batch holds (rescore_corpus loops).
No length lies in 129 .. 192 or 257 .. 384, so every pass of every entry point runs at padded length 64, 128 or 256, where a row's bits do not depend on the batch
it travels in (tests/test_gpu_parity.py::test_full_batch_properties): the two engines must agree byte for byte, and on every counter.  This is an equality between
two runs of the code under test; it means something next to the suites named above, which pin the roomy engine to the safe and default engines' bytes and to the
float64 references."""
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
import test_guarded_form_gpu as gg  # noqa: E402  (the mixed case of the 12-layer sink model)
import test_sink_routing_gpu as rs  # noqa: E402  (the sweep in the caller's row order, the list)
import test_sink_routing_cpu as rc  # noqa: E402  (the numpy restatement of the routing rule)

CASE = "mid_all_80_3001"
LENS = [16, 230, 40, 256, 64, 250, 100, 120, 128, 110, 200, 60, 256, 30, 225, 90]
BANK_ROWS = [0, 6, 1, 7]  # two marked anchors and the same two unmarked, interleaved, in ONE call
ROOMY = dict(max_tokens=16 * 512, max_batch=16)
TIGHT = dict(max_tokens=4 * 256, max_batch=8)
COUNTERS = ("forms", "route", "stats", "items")


@pytest.fixture(scope="module")
def refs(golden_dir):
    return np.load(os.path.join(golden_dir, "guarded_form_refs.npz")), np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))


def _batch(vocab):
    """gg._ragged_batch with the lengths of this module: every even row marked."""
    lens = np.array(LENS, np.int32)
    assert not (((lens >= 129) & (lens <= 192)) | ((lens >= 257) & (lens <= 384))).any()
    ids, _ = synth.make_ids(len(lens), 256, vocab, seed=synth.SEED + 77, ragged=False)
    ids[ids == synth.MID_ID] = synth.MID_ID + 1
    ids = (ids * (np.arange(256)[None, :] < lens[:, None])).astype(np.int32)
    marked = np.arange(0, len(lens), 2)
    ids[marked] = synth.mark_mid_token(ids[marked], lens[marked])
    return np.ascontiguousarray(ids), lens, marked


def _engine(dims, w, compute, size, tokens=None):
    from memvul_amd.binding import Engine

    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_anchors=16, **size)
    eng.load_state_dict(w, compute)
    if tokens is not None:
        eng.set_sink_tokens(tokens)
    return eng


def _append_bank(eng, aids, alens):
    L = int(alens[BANK_ROWS].max())
    assert L <= 128  # (one pass at padded length 64 or 128 on either engine)
    eng.anchor_reset()
    eng.anchor_append(np.ascontiguousarray(aids[BANK_ROWS, :L]), np.ascontiguousarray(alens[BANK_ROWS]))
    return eng.anchor_get()


def _halves(eng, ids, lens):
    """Two tickets in flight: the batch and the batch reversed (B <= max_batch is required there)."""
    t1 = eng.forward_by_length_begin(ids, lens, want_embed=True, min_tokens=1)
    t2 = eng.forward_by_length_begin(ids[::-1].copy(), lens[::-1].copy(), want_embed=True, min_tokens=1)
    assert t1[0] == "pending" and t2[0] == "pending"
    r1 = eng.forward_by_length_end(t1)
    f1 = eng.last_row_forms()
    r2 = eng.forward_by_length_end(t2)
    out = {"first_" + k: v for k, v in r1.items()}
    out.update({"second_" + k: v for k, v in r2.items()})
    out["forms"] = f1 + eng.last_row_forms()
    return out


def _flat_sweep(eng, ids, lens):
    """The whole corpus in its own order at 256 tokens, in batches of 4, P(same) kept: eight marked rows pend at ONE width."""
    eng.set_streams(2)
    eng.corpus_upload(ids, lens)
    eng.corpus_run(0, len(lens), 4, keep_probs=True, s_eff=256)
    best, idx, ps = eng.corpus_results(0, len(lens), with_probs=True)
    return {"best": best, "best_idx": idx, "ps": ps, "forms": eng.corpus_row_forms(0, len(lens))}


def _every_entry_point(eng, ids, lens, aids, alens, bank_safe):
    """{entry point: {every output array, "forms", "route", "stats", "items"}}, the counters those of that call alone."""
    res = {}

    def call(name, fn):
        eng.route_stats(reset=True)
        eng.form_stats(reset=True)
        eng.attention_concentration(reset=True)
        out = dict(fn())
        if "forms" not in out:
            out["forms"] = eng.last_row_forms()
        out.update(route=eng.route_stats(), stats=eng.form_stats(), items=eng.attention_concentration()[2])
        res[name] = out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the guarded form warns about the rescored share)
        call("anchor_append", lambda: {"bank": _append_bank(eng, aids, alens)})
        call("forward", lambda: eng.forward(ids, lens, want_embed=True))
        call("encode", lambda: {"embed": eng.encode(ids, lens)})
        call("forward_by_length", lambda: eng.forward_by_length(ids, lens, want_embed=True, min_tokens=1))
        call("begin_end", lambda: _halves(eng, np.ascontiguousarray(ids[:8]), np.ascontiguousarray(lens[:8])))
        eng.anchor_set(bank_safe)
        for streams in (2, 1):
            for with_probs in (False, True):
                call(f"sweep_{streams}_{int(with_probs)}", lambda: rs._sweep(eng, ids, lens, streams, with_probs))
        call("sweep_flat_256", lambda: _flat_sweep(eng, ids, lens))
    return res


_shared = {}


def _setup(refs):
    if not _shared:
        dims, w, _, _, aids, alens, _, _ = gg._mixed(refs, CASE)
        ids, lens, marked = _batch(dims.vocab_size)
        assert np.flatnonzero(rc.rule(ids, lens, rs.LIST)).tolist() == marked.tolist()
        assert np.flatnonzero(rc.rule(aids[BANK_ROWS], alens[BANK_ROWS], rs.LIST)).tolist() == [0, 2]
        srt = np.sort(lens)
        assert (-(-srt[3::4] // 64) * 64).tolist() == [64, 128, 256, 256]  # the padded lengths of the sweep's batches of 4, sorted by length
        eng = _engine(dims, w, "safe", ROOMY)
        try:
            bank_safe = _append_bank(eng, aids, alens)
        finally:
            eng.close()
        _shared.update(dims=dims, w=w, aids=aids, alens=alens, ids=ids, lens=lens, marked=marked, bank_safe=bank_safe)
    return _shared


@pytest.mark.parametrize("tokens", [rs.LIST, None], ids=["with_the_list", "without_the_list"])
def test_a_tight_engine_agrees_with_a_roomy_one(refs, tokens):
    """anchor_append (four in one call), forward and encode at S = 256, forward_by_length, its two halves with two tickets in flight on the first 8 rows and on
    those rows reversed, bucketed_sweep(batch=4) at 2 and at 1 streams with and without P(same), and one sweep of all 16 rows at 256 tokens: the tight engine and
    the roomy one agree on every output array byte for byte, on the row forms, on form_stats(), route_stats() and the monitor's item total; every marked row says
    safe."""
    sh = _setup(refs)
    got = {}
    for name, size in (("roomy", ROOMY), ("tight", TIGHT)):
        eng = _engine(sh["dims"], sh["w"], "guarded", size, tokens)
        try:
            got[name] = _every_entry_point(eng, sh["ids"], sh["lens"], sh["aids"], sh["alens"], sh["bank_safe"])
        finally:
            eng.close()
    marked = sh["marked"]
    assert list(got["tight"]) == list(got["roomy"])
    for name, t in got["tight"].items():
        r = got["roomy"][name]
        print(f"{name}: forms safe {sum(f == 'safe' for f in t['forms'])} of {len(t['forms'])}, route {t['route']}, stats {t['stats']}, items {t['items']}")
        assert set(t) == set(r), name
        for k in t:
            if k in COUNTERS:
                assert t[k] == r[k], (name, k, t[k], r[k])
            else:
                assert t[k].dtype == r[k].dtype and t[k].shape == r[k].shape and t[k].tobytes() == r[k].tobytes(), (name, k)
        forms = np.array(t["forms"])
        if name == "anchor_append":
            m = [0, 2]
        elif name == "begin_end":  # rows 0 .. 7, then the same rows reversed
            m8 = marked[marked < 8]
            m = np.concatenate([m8, 8 + (7 - m8)])
        else:
            m = marked
        assert (forms[m] == "safe").all(), (name, forms)
        assert t["route"] == (len(m) if tokens else 0), (name, t["route"])
