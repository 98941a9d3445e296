"""Re-matching a resident corpus against a changed anchor bank, on the GPU (include/memvul_hip.h mv_corpus_keep / mv_corpus_rematch / mv_corpus_embeddings /
mv_corpus_topk).  A corpus that keeps its embeddings is matched again without the encoder; the property everything is held to is the matcher's own (match_topk.h:
a (report, anchor) result depends neither on the batch nor on the chunking): a full rematch is BYTE-equal to sweeping again, an appended one to the full one.
There is no tolerance in this file."""
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

L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0)  # the peaked 2-layer model of tests/test_gpu_kernels.py
N, BATCH, S = 48, 16, 256
MATCHER_CLASSES = {"match", "topk"}


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


def _corpus(vocab):
    """48 ragged rows at S = 256, sorted by length as bucketed_sweep uploads them, and the s_eff of each batch of 16 as it sets it."""
    rng = np.random.default_rng(synth.SEED + 4801)
    lens = np.concatenate([[3, 15, 16, 17, 64, 65, 192, 256], rng.integers(4, 257, N - 8)]).astype(np.int32)
    ids, _ = synth.make_ids(N, S, vocab, seed=synth.SEED + 48, ragged=False)
    ids = np.ascontiguousarray(ids * (np.arange(S)[None, :] < lens[:, None]), np.int32)
    order = np.argsort(lens, kind="stable")
    ids, lens = np.ascontiguousarray(ids[order]), np.ascontiguousarray(lens[order])
    return ids, lens, [int(lens[s0 + BATCH - 1]) for s0 in range(0, N, BATCH)]


def _anchors(vocab, n, seed):
    return synth.make_ids(n, 64, vocab, seed=synth.SEED + seed, ragged=True, min_len=16)


def _runs(eng, s_effs, keep_probs=False, count=N):
    for b, s0 in enumerate(range(0, count, BATCH)):
        eng.corpus_run(s0, BATCH, BATCH, keep_probs=keep_probs, s_eff=s_effs[b])


def _sweep(eng, ids, lens, s_effs, keep=None, keep_probs=False):
    eng.corpus_upload(ids, lens)
    if keep is not None:
        eng.corpus_keep(*keep)
    _runs(eng, s_effs, keep_probs)
    return eng.corpus_results(0, len(lens), with_probs=keep_probs)


def _same(a, b, what):
    for x, y, name in zip(a, b, what):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), name


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("streams", [2, 1])
@pytest.mark.parametrize("compute", ["precise", "f16"])
def test_kept_embeddings_are_the_sweeps_own(gu, compute, streams):
    """1. corpus_embeddings is byte-equal to forward(..., want_embed=True) on the same 16-row batches at the same width, and keeping changes nothing of what the
    sweep returned before: best / best_idx are byte-equal to the same upload and runs on an engine that keeps nothing."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the peaked model trips the sink warning of the default form)
        eng = gu.engine_for(L2, WK, compute_dtype=compute, env={"MEMVUL_STREAMS": "1"} if streams == 1 else None)
        dims, _ = gu.weights_for(L2, WK)
        ids, lens, s_effs = _corpus(dims.vocab_size)
        eng.anchor_reset()
        eng.anchor_append(*_anchors(dims.vocab_size, 5, 1))
        plain = _sweep(eng, ids, lens, s_effs)
        kept = _sweep(eng, ids, lens, s_effs, keep=(True, 3))
        emb = eng.corpus_embeddings(0, N)
        tp, ti = eng.corpus_topk(0, N)
        fw = [eng.forward(ids[s0:s0 + BATCH, :s_effs[b]], lens[s0:s0 + BATCH], want_logits=False, want_probs=False, want_embed=True)
              for b, s0 in enumerate(range(0, N, BATCH))]
        eng.anchor_reset()
    _same(kept[:2], plain[:2], ("best", "best_idx"))
    want = np.concatenate([o["embed"] for o in fw])
    gu.record("rematch_kept_embeddings", compute=compute, streams=streams, rows_differing=int((emb != want).any(axis=1).sum()),
              best_rows_differing=int((kept[0] != plain[0]).any(axis=1).sum()))
    assert emb.tobytes() == want.tobytes()
    _same((kept[0], kept[1]), (np.concatenate([o["best"] for o in fw]), np.concatenate([o["best_idx"] for o in fw])), ("forward best", "forward best_idx"))
    assert ti[:, 0].tobytes() == kept[1].tobytes() and tp[:, 0].tobytes() == kept[0][:, 0].tobytes()  # (same_idx = 0: the first entry of a list is the best anchor)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_full_rematch_equals_sweeping_again(gu):
    """2. 5 anchors -> sweep -> append 4 -> corpus_rematch(0, 48, 0, keep_probs=True): best, best_idx, P(same) and top-3 are byte-equal to running the same three
    corpus_run calls again, and the per-class profile around the rematch shows launches of the matcher classes only (max_batch = 32: two batches)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = gu.engine_for(L2, WK, compute_dtype="precise", max_batch=32)
        dims, _ = gu.weights_for(L2, WK)
        ids, lens, s_effs = _corpus(dims.vocab_size)
        eng.anchor_reset()
        eng.anchor_append(*_anchors(dims.vocab_size, 5, 1))
        first = _sweep(eng, ids, lens, s_effs, keep=(True, 3), keep_probs=True)
        emb = eng.corpus_embeddings(0, N)
        eng.anchor_append(*_anchors(dims.vocab_size, 4, 2))
        eng.sync()
        eng.profile_enable(True)
        eng.profile_read()
        eng.corpus_rematch(0, N, 0, keep_probs=True)
        prof = eng.profile_read()
        eng.profile_enable(False)
        got = eng.corpus_results(0, N, with_probs=True) + eng.corpus_topk(0, N)
        assert eng.corpus_embeddings(0, N).tobytes() == emb.tobytes()
        _runs(eng, s_effs, keep_probs=True)
        want = eng.corpus_results(0, N, with_probs=True) + eng.corpus_topk(0, N)
        eng.anchor_reset()
    launched = {k: v[1] for k, v in prof.items() if v[1]}
    gu.record("rematch_full_profile", launches=launched, match_ms=prof["match"][0])
    assert set(launched) <= MATCHER_CLASSES and launched.get("match") == 2, launched
    assert got[2].shape == (N, 9) and first[2].shape == (N, 5)
    assert got[2][:, :5].tobytes() == first[2].tobytes()  # (the first five anchors are the ones the first sweep saw)
    _same(got, want, ("best", "best_idx", "p_same", "topk_p", "topk_idx"))


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def _bank(P):
    rng = np.random.default_rng(synth.SEED + 303)
    return rng.standard_normal((303, P)).astype(np.float32)


def test_appended_equals_full_across_both_chunk_widths(gu):
    """3. 120 anchors (one 128-anchor chunk) swept with k = 10, then 300 whose first 120 are the same bytes (two 256-anchor chunks; the slice of 180 is one): the
    appended rematch from g_first = 120 on one engine is byte-equal to the full rematch on a second, identical one.  Row 7 is copied to rows 130 and 131 (the
    stored, lower index wins the tie, then 130 before 131) and row 200 is NaN (ranks first).  Then 300 -> 303 (a slice smaller than k), and g_first == G."""
    from memvul_amd.binding import Engine

    dims, w = gu.weights_for(L2, WK)
    ids, lens, s_effs = _corpus(dims.vocab_size)
    K = 10
    engs = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                e = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_pos=dims.max_pos, max_tokens=16384, max_batch=32, max_anchors=320)
                e.load_state_dict(w, "precise")
                engs.append(e)
            a, b = engs
            bank = _bank(a.P)
            # row 7 = the anchor most reports rank first among the first 120, so that its copies tie at the head of the lists
            a.anchor_set(bank[:120])
            idx0 = _sweep(a, ids, lens, s_effs)[1]
            top = int(np.bincount(idx0, minlength=120).argmax())
            bank[[7, top]] = bank[[top, 7]]
            bank[130] = bank[131] = bank[7]
            bank[200] = np.nan
            for e in engs:
                e.anchor_set(bank[:120])
                _sweep(e, ids, lens, s_effs, keep=(True, K))
                e.anchor_set(bank[:300])
            a.corpus_rematch(0, N, 120, False)
            b.corpus_rematch(0, N, 0, False)
            ra = a.corpus_results(0, N) [:2] + a.corpus_topk(0, N)
            rb = b.corpus_results(0, N)[:2] + b.corpus_topk(0, N)
            ti = ra[3]
            tied = int(sum(1 for r in range(N) if [7, 130, 131] in [ti[r, j:j + 3].tolist() for j in range(K - 2)]))
            gu.record("rematch_appended_vs_full", rows_differing=int(sum(x.tobytes() != y.tobytes() for x, y in zip(ra[3], rb[3]))), rows_with_the_tie=tied,
                      nan_first=int((ti[:, 0] == 200).sum()))
            _same(ra, rb, ("best", "best_idx", "topk_p", "topk_idx"))
            assert (ti[:, 0] == 200).all() and np.isnan(ra[2][:, 0]).all() and (ra[1] == 200).all() and np.isnan(ra[0][:, 0]).all()
            assert tied >= 1, "the duplicated anchor is in no list: the tie across the split was not exercised"
            for r in range(N):  # wherever the copies appear they follow the stored anchor, in index order
                row = ti[r].tolist()
                pos = [row.index(g) for g in (7, 130, 131) if g in row]
                assert pos == sorted(pos) and (131 not in row or 130 in row) and (130 not in row or 7 in row), row
            # a slice smaller than k
            for e in engs:
                e.anchor_set(bank[:303])
            a.corpus_rematch(0, N, 300, False)
            b.corpus_rematch(0, N, 0, False)
            ra = a.corpus_results(0, N)[:2] + a.corpus_topk(0, N)
            rb = b.corpus_results(0, N)[:2] + b.corpus_topk(0, N)
            _same(ra, rb, ("best", "best_idx", "topk_p", "topk_idx"))
            # g_first == G: nothing was appended
            a.corpus_rematch(0, N, 303, False)
            _same(a.corpus_results(0, N)[:2] + a.corpus_topk(0, N), ra, ("best", "best_idx", "topk_p", "topk_idx"))
    finally:
        for e in engs:
            e.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_guarded_form_and_routed_rows_carry_the_kept_columns(gu, golden_dir):
    """4. mid_all_80_3001 (12 layers, 16 reports at S = 256, rows 0 .. 7 carry the sink): a guarded engine with the first 6 anchors runs a keeping sweep; the rows
    it rescored hold the embedding the safe form's encode gives them at that width, the others the default form's; after the other 6 anchors are appended, the
    appended rematch is byte-equal to a fresh guarded sweep against all 12.  Then once more with the sink token on the list: the marked rows run in no
    default-form pass, the batch is a split one, and its indexed pass carries the columns.  (One handle: the three forms are the same weights and planes, only
    the per-pass choices differ — the safe and the default form's encode are taken from it before it is put into the guarded form.)"""
    import test_guarded_form_gpu as gg
    from memvul_amd.binding import Engine

    refs = (None, np.load(os.path.join(golden_dir, "r06_sink_refs.npz")))
    dims, w, ids, lens, aids, alens, marked, _ = gg._mixed(refs, "mid_all_80_3001")  # (shared with that module's tests: the case is made once per session)
    B, K = len(lens), 3
    aw = int(alens.max())
    g = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=16 * 512, max_batch=16, max_anchors=16)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g.load_state_dict(w, "safe")
            e_safe = g.encode(ids, lens)
            g.set_form("default")
            e_def = g.encode(ids, lens)
            g.set_form("guarded")
            g.form_stats(reset=True)

            def append(first):  # six anchors per call, the same calls on both sides of every comparison
                g.anchor_append(aids[first:first + 6, :aw], alens[first:first + 6])

            def sweep(n_anchors):
                g.anchor_reset()
                for first in range(0, n_anchors, 6):
                    append(first)
                g.corpus_upload(ids, lens)
                g.corpus_keep(True, K)
                g.corpus_run(0, B, B)
                return g.corpus_results(0, B)[:2] + g.corpus_topk(0, B)

            for listed in (False, True):
                g.set_sink_tokens([synth.MID_ID] if listed else [])
                sweep(6)
                forms = np.array(g.corpus_row_forms(0, B))
                emb = g.corpus_embeddings(0, B)
                assert (forms[marked] == "safe").all(), forms
                assert g.corpus_route_flags(0, B).tolist() == [listed and r in marked for r in range(B)]
                for r in range(B):
                    assert emb[r].tobytes() == (e_safe if forms[r] == "safe" else e_def)[r].tobytes(), (listed, r, forms[r])
                append(6)
                g.corpus_rematch(0, B, 6, False)
                got = g.corpus_results(0, B)[:2] + g.corpus_topk(0, B) + (g.corpus_embeddings(0, B),)
                want = sweep(12) + (g.corpus_embeddings(0, B),)
                gu.record("rematch_guarded", listed=listed, rescored=int((forms == "safe").sum()),
                          rows_differing=int(sum(x.tobytes() != y.tobytes() for x, y in zip(got[3], want[3]))))
                _same(got, want, ("best", "best_idx", "topk_p", "topk_idx", "embed"))
    finally:
        g.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_strictness(gu):
    """5. Every misuse returns its stated code with a message, and corpus_results afterwards returns the unchanged results."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = gu.engine_for(L2, WK, compute_dtype="precise")
        dims, _ = gu.weights_for(L2, WK)
        ids, lens, s_effs = _corpus(dims.vocab_size)
        eng.anchor_reset()
        eng.anchor_append(*_anchors(dims.vocab_size, 5, 1))

        def refused(code, words, call):
            before = eng.corpus_results(0, N)
            with pytest.raises(RuntimeError, match=r"\(%d\): .*%s" % (code, words)):
                call()
            _same(eng.corpus_results(0, N)[:2], before[:2], ("best", "best_idx"))

        INVALID, STATE = -1, -3
        plain = _sweep(eng, ids, lens, s_effs)
        refused(STATE, "swept already", lambda: eng.corpus_keep(True, 0))                # keep after a run
        refused(STATE, "mv_corpus_keep", lambda: eng.corpus_rematch(0, N, 0, False))     # nothing kept
        refused(STATE, "mv_corpus_keep", lambda: eng.corpus_embeddings(0, N))
        refused(STATE, "mv_corpus_keep", lambda: eng.corpus_topk(0, N))
        eng.corpus_upload(ids, lens)
        refused(INVALID, "64", lambda: eng.corpus_keep(True, 65))                        # topk of 65
        refused(INVALID, "0 or 1", lambda: eng._check(eng._lib.mv_corpus_keep(eng._h, 2, 0), "mv_corpus_keep"))
        eng.corpus_keep(True, 6)
        refused(INVALID, "exceeds the number of anchors", lambda: _runs(eng, s_effs))    # k larger than the bank at run time
        eng.corpus_keep(True, 3)                                                         # (nothing has run: it may still be set)
        _runs(eng, s_effs, count=BATCH)
        refused(STATE, "row 16", lambda: eng.corpus_rematch(0, N, 0, False))             # a row no keeping run covered
        refused(STATE, "row 16", lambda: eng.corpus_embeddings(BATCH, 1))
        refused(STATE, "row 16", lambda: eng.corpus_topk(0, N))
        _runs(eng, s_effs)
        _same(eng.corpus_results(0, N)[:2], plain[:2], ("best", "best_idx"))
        refused(INVALID, "g_first", lambda: eng.corpus_rematch(0, N, -1, False))         # g_first outside [0, G]
        refused(INVALID, "g_first", lambda: eng.corpus_rematch(0, N, 6, False))
        refused(INVALID, "keep_probs", lambda: eng.corpus_rematch(0, N, 2, True))        # keep_probs with g_first > 0
        refused(INVALID, "bad range", lambda: eng.corpus_rematch(40, 9, 0, False))
        eng.corpus_rematch(0, N, 5, False)                                               # g_first == G: MV_OK, nothing changes
        _same(eng.corpus_results(0, N)[:2], plain[:2], ("best", "best_idx"))
        eng.anchor_reset()
        refused(STATE, "anchor bank is empty", lambda: eng.corpus_rematch(0, N, 0, False))  # no anchors
        eng.anchor_append(*_anchors(dims.vocab_size, 2, 3))
        refused(INVALID, "exceeds the number of anchors", lambda: eng.corpus_rematch(0, N, 0, False))  # the kept k = 3 against 2 anchors
        eng.anchor_reset()
