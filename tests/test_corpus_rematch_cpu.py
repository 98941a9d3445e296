"""Re-matching a resident corpus against a changed anchor bank (include/memvul_hip.h mv_corpus_keep / mv_corpus_rematch / mv_corpus_embeddings /
mv_corpus_topk), the parts that need no GPU: the ABI in all three places, the merge rule of the appended mode restated in numpy against a plain sort, and the
host logic of binding.Engine / ModelMemory against the recording stand-in library of tests/test_safe_form_cpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from memvul_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_abi  # noqa: E402
import test_safe_form_cpu as sf  # noqa: E402

NAMES = ("mv_corpus_keep", "mv_corpus_rematch", "mv_corpus_embeddings", "mv_corpus_topk")


# ---- header, binding, exports ------------------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_carry_the_four_entries():
    from memvul_amd import build

    declared = test_abi._declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    build.build(verbose=False)
    lib = binding.load_library()
    for name in NAMES:
        assert name in declared and name in binding.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^int %s\(mv_handle\* h, " % name, hdr, flags=re.M), name
    assert declared == sorted(binding.ABI_SYMBOLS)
    vp = C.c_void_p
    assert lib.mv_corpus_keep.argtypes == [vp, C.c_int, C.c_int]
    assert lib.mv_corpus_rematch.argtypes == [vp, C.c_int64, C.c_int64, C.c_int, C.c_int]
    assert lib.mv_corpus_embeddings.argtypes == [vp, C.c_int64, C.c_int64, vp]
    assert lib.mv_corpus_topk.argtypes == [vp, C.c_int64, C.c_int64, vp, vp]
    assert "model_memory.py:105-115" in hdr[hdr.index("the editable memory"):hdr.index("int mv_corpus_keep(")]
    assert "model_memory.py:135-147" in hdr[hdr.index("the editable memory"):hdr.index("int mv_corpus_keep(")]
    # the four are function-try-blocks like every other entry (test_abi checks the whole file; here: they are in it)
    from stage_kit import host_source

    src = host_source()
    for name in NAMES:
        assert re.search(r"^int %s\([^{;]*\) try \{" % name, src, flags=re.M), name


# ---- the merge rule ----------------------------------------------------------------------------------------------------------------------------------------------
# The matcher's order (match_topk.h): key = P(same), NaN ranking above every probability (mk_key), largest key first, a tie to the lower GLOBAL anchor index.

EXHAUSTED = 0x7fffffff


def key(p):
    p = np.asarray(p, np.float32)
    return np.where(np.isnan(p), np.float32(2.0), p)


def plain(ps, pq, k):
    """Sort all G candidates by (key desc, index asc): best [2], best index, top-k (P(same), index)."""
    order = np.lexsort((np.arange(len(ps)), -key(ps).astype(np.float64)))
    top = order[:k]
    return np.array([ps[order[0]], pq[order[0]]], np.float32), int(order[0]), ps[top].copy(), top.astype(np.int32)


def merge(best_old, idx_old, topk_old, best_new, idx_new, topk_new, g_first, k):
    """The rule of rematch_merge_kernel.  topk_* = (P(same) [n], index [n]) lists, each in the matcher's order; the slice's indices are relative to g_first."""
    best, idx = best_old.copy(), idx_old
    if key(best_new[0]) > key(best_old[0]):  # strictly: on a tie the stored, lower index stays
        best, idx = best_new.copy(), g_first + idx_new
    po, io = topk_old
    pn, in_ = topk_new[0], topk_new[1] + g_first
    out_p, out_i = np.full(k, -1.0, np.float32), np.full(k, EXHAUSTED, np.int32)

    def beats(pa, ia, pb, ib):  # (key desc, index asc)
        return key(pa) > key(pb) or (key(pa) == key(pb) and ia < ib)

    for l in range(len(po)):  # rank = own position + the entries of the other list that beat it
        r = l + sum(beats(pn[j], in_[j], po[l], io[l]) for j in range(len(pn)))
        if r < k:
            assert out_i[r] == EXHAUSTED
            out_p[r], out_i[r] = po[l], io[l]
    for l in range(len(pn)):
        r = l + sum(beats(po[j], io[j], pn[l], in_[l]) for j in range(len(po)))
        if r < k:
            assert out_i[r] == EXHAUSTED
            out_p[r], out_i[r] = pn[l], in_[l]
    return best, idx, out_p, out_i


def _check_split(ps, pq, n_old, k):
    G = len(ps)
    bo, io, tpo, tio = plain(ps[:n_old], pq[:n_old], min(k, n_old))
    ks = min(k, G - n_old)
    bn, in_, tpn, tin = plain(ps[n_old:], pq[n_old:], ks)
    # a stored list is full (k <= the anchors it was computed against is enforced at run time) unless this case asks for fewer old anchors than k
    got = merge(bo, io, (tpo, tio), bn, in_, (tpn, tin), n_old, min(k, G))
    want = plain(ps, pq, min(k, G))
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (n_old, G, k)
    assert got[2].tobytes() == want[2].tobytes() and got[3].tolist() == want[3].tolist(), (n_old, G, k, got[3], want[3])


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("sizes", [(3, 1), (120, 180), (64, 3)])
def test_merge_equals_sorting_all_candidates(k, sizes):
    n_old, n_new = sizes
    G = n_old + n_new
    for seed in range(6):
        rng = np.random.default_rng(1000 * k + 10 * n_old + seed)
        ps = rng.random(G).astype(np.float32)
        if seed >= 1:  # exact ties: inside the old side, inside the new side and across the split
            ps = np.round(ps * 4).astype(np.float32) / 4
            ps[n_old] = ps[n_old - 1] = ps[0]
        if seed == 2:
            ps[rng.integers(0, n_old)] = np.nan
        if seed == 3:
            ps[n_old + rng.integers(0, n_new)] = np.nan
        if seed == 4:  # on both sides: the lower index first
            ps[n_old - 1] = ps[G - 1] = np.nan
        if seed == 5:
            ps[:] = 0.5
        pq = (1 - ps).astype(np.float32)
        _check_split(ps, pq, n_old, k)


def test_merge_slice_smaller_than_k_and_tie_order():
    ps = np.array([0.1, 0.9, 0.3, 0.9, 0.2, 0.9, 0.9], np.float32)  # old = 4 anchors, new = 3; k = 5 > 3
    bo, io, tpo, tio = plain(ps[:4], 1 - ps[:4], 4)
    bn, in_, tpn, tin = plain(ps[4:], 1 - ps[4:], 3)
    best, idx, tp, ti = merge(bo, io, (tpo, tio), bn, in_, (tpn, tin), 4, 5)
    assert idx == 1 and ti.tolist() == [1, 3, 5, 6, 2] and tp.tolist() == [np.float32(0.9)] * 4 + [np.float32(0.3)]
    assert best.tobytes() == np.array([ps[1], 1 - ps[1]], np.float32).tobytes()


# ---- Engine host logic -------------------------------------------------------------------------------------------------------------------------------------------

class _Lib(sf._Lib):
    """The recorder of tests/test_safe_form_cpu.py plus the four entries: results carry the row number, so that a permutation is visible."""

    def mv_corpus_upload(self, h, ids, lens, n, S):
        self.n_rows, self.k = n, 0
        return super().mv_corpus_upload(h, ids, lens, n, S)

    def mv_corpus_keep(self, h, embed, topk):
        self.log.append(("keep", embed, topk))
        self.k = topk
        return 0

    def mv_corpus_rematch(self, h, first, count, g_first, keep_probs):
        self.log.append(("rematch", first, count, g_first, keep_probs))
        return 0

    def mv_corpus_results(self, h, first, count, best, idx, ps):
        self.log.append(("results", first, count))
        b, i = C.cast(best, C.POINTER(C.c_float)), C.cast(idx, C.POINTER(C.c_int32))
        for r in range(count):
            b[2 * r], b[2 * r + 1], i[r] = float(first + r), 0.0, first + r
        if ps:
            p = C.cast(ps, C.POINTER(C.c_float))
            for r in range(count * self.n_anchors):
                p[r] = float(first + r // self.n_anchors)
        return 0

    def mv_corpus_topk(self, h, first, count, p, i):
        self.log.append(("topk", first, count))
        pp, ii = C.cast(p, C.POINTER(C.c_float)), C.cast(i, C.POINTER(C.c_int32))
        for r in range(count * self.k):
            pp[r], ii[r] = float(first + r // self.k), first + r // self.k
        return 0


LENS = np.array([30, 200, 60, 256, 100, 130, 250, 40], np.int32)


def _engine(monkeypatch, on_sink=None, **kw):
    if on_sink:
        monkeypatch.setenv("MEMVUL_ON_SINK", on_sink)
    else:
        monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    lib = _Lib(**kw)
    return lib, sf.StandInEngine(lib)


def _rematches(lib):
    return [c for c in lib.log if c[0] == "rematch"]


def test_g_first_after_append_only_growth_and_the_original_order(monkeypatch):
    lib, eng = _engine(monkeypatch, sink_share=0.0)
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    best, idx, _ = eng.bucketed_sweep(sf.IDS, LENS, 4, keep=True, topk=3)
    assert ("keep", 1, 3) in lib.log and lib.log.index(("keep", 1, 3)) == lib.log.index(("upload", 8, 256)) + 1
    order = np.argsort(LENS, kind="stable")
    assert idx[order].tolist() == list(range(8))  # (original row order[j] is corpus row j)
    eng.anchor_append(sf.IDS[:2], sf.LENS[:2])
    eng.anchor_append(sf.IDS[:1], sf.LENS[:1])
    best, idx, ps = eng.rematch_sweep()
    assert _rematches(lib) == [("rematch", 0, 8, 5, 0)] and ps is None
    assert idx[order].tolist() == list(range(8)) and best[order][:, 0].tolist() == list(range(8))
    tp, ti = eng.sweep_topk()
    assert tp.shape == (8, 3) and ti[order][:, 0].tolist() == list(range(8)) and tp[order][:, 2].tolist() == list(range(8))
    # the stored results now cover 8 anchors: growing again starts there, and nothing new is a no-op the library is told about as g_first == G
    eng.anchor_append(sf.IDS[:3], sf.LENS[:3])
    eng.rematch_sweep()
    eng.rematch_sweep()
    assert _rematches(lib)[1:] == [("rematch", 0, 8, 8, 0), ("rematch", 0, 8, 11, 0)]


def test_g_first_is_zero_after_set_after_reset_and_with_probs(monkeypatch):
    lib, eng = _engine(monkeypatch, sink_share=0.0)
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    eng.bucketed_sweep(sf.IDS, LENS, 4, keep=True)
    eng.anchor_set(np.zeros((7, 512), np.float32))  # more anchors than before, but not the same ones
    eng.rematch_sweep()
    eng.anchor_reset()
    eng.anchor_append(sf.IDS[:8], sf.LENS[:8])
    eng.rematch_sweep()
    eng.anchor_append(sf.IDS[:1], sf.LENS[:1])
    order = np.argsort(LENS, kind="stable")
    best, idx, ps = eng.rematch_sweep(with_probs=True)  # append-only since the last rematch, but P(same) changes its pitch
    assert ps.shape == (8, 9) and ps[order][:, 0].tolist() == list(range(8))
    eng.anchor_append(sf.IDS[:1], sf.LENS[:1])
    eng.rematch_sweep()
    assert _rematches(lib) == [("rematch", 0, 8, 0, 0), ("rematch", 0, 8, 0, 0), ("rematch", 0, 8, 0, 1), ("rematch", 0, 8, 9, 0)]
    # a bank that shrank is never "appended to"
    lib2, eng2 = _engine(monkeypatch, sink_share=0.0)
    eng2.anchor_append(sf.IDS[:5], sf.LENS[:5])
    eng2.bucketed_sweep(sf.IDS, LENS, 4, keep=True)
    lib2.n_anchors = 3
    eng2.rematch_sweep()
    assert _rematches(lib2) == [("rematch", 0, 8, 0, 0)]


def test_g_first_is_zero_after_an_on_sink_trip(monkeypatch):
    import warnings

    lib, eng = _engine(monkeypatch, on_sink="safe", items=60, sink_share=0.0)
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    eng.bucketed_sweep(sf.IDS, LENS, 8, keep=True)
    assert eng.form == "default"
    lib.sink_share = 1.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eng.anchor_append(sf.IDS[:2], sf.LENS[:2])  # trips: the whole bank is encoded again in the safe form
    assert eng.form == "safe" and len(sf._told(rec, "SAFE form")) == 1 and eng.n_anchors == 7
    eng.rematch_sweep()
    assert _rematches(lib) == [("rematch", 0, 8, 0, 0)]
    eng.anchor_append(sf.IDS[:1], sf.LENS[:1])
    eng.rematch_sweep()
    assert _rematches(lib)[1:] == [("rematch", 0, 8, 7, 0)]


def test_an_engine_that_never_keeps_makes_no_new_call(monkeypatch):
    lib, eng = _engine(monkeypatch, sink_share=0.0)
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    eng.bucketed_sweep(sf.IDS, LENS, 4)
    eng.bucketed_sweep(sf.IDS, LENS, 4, with_probs=True)
    eng.anchor_set(np.zeros((2, 512), np.float32))
    eng.anchor_reset()
    assert {c[0] for c in lib.log} <= {"anchor_append", "upload", "run", "results", "anchor_set", "anchor_reset", "concentration"}  # what it called before
    with pytest.raises(RuntimeError, match="keep=True"):
        eng.rematch_sweep()
    with pytest.raises(RuntimeError, match="topk=k"):
        eng.sweep_topk()
    # top-k alone keeps no embeddings: rematch_sweep says so before any library call
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    eng.bucketed_sweep(sf.IDS, LENS, 4, topk=2)
    assert ("keep", 0, 2) in lib.log
    with pytest.raises(RuntimeError, match="keep=True"):
        eng.rematch_sweep()
    assert not _rematches(lib)


# ---- ModelMemory -------------------------------------------------------------------------------------------------------------------------------------------------

class _Vocab:
    def get_token_index(self, token, namespace=None):
        return {"same": 0, "diff": 1}[token]


class _Metric:
    def __init__(self):
        self.calls = []

    def add_arrays(self, same, score):
        self.calls.append((same.copy(), score.copy()))


class _OldEngine:
    """An engine from before this feature: bucketed_sweep takes neither keep nor topk."""

    def bucketed_sweep(self, ids, lens, batch, with_probs=False):
        n = len(lens)
        return np.zeros((n, 2), np.float32), np.zeros(n, np.int32), None


def _model(engine):
    from memvul_amd.kept_sweep import KeptSweepState
    from memvul_amd.model_memory import ModelMemory

    m = ModelMemory.__new__(ModelMemory)
    counts = []
    d = m.__dict__
    d.update(_engine=engine, vocab=_Vocab(), _label_namespace="labels", _same_idx=0, _siamese_metric=_Metric(), _counts=lambda best, lab: counts.append((best.copy(), lab.copy())),
             _kept=KeptSweepState())
    return m, counts


def test_rematch_arrays_needs_a_kept_sweep_and_scores_like_sweep_arrays(monkeypatch):
    arrays = {"type": "test", "ids": sf.IDS, "lens": LENS, "same": np.array([1, 0, 0, 1, 0, 0, 0, 1], bool)}
    lib, eng = _engine(monkeypatch, sink_share=0.0)
    eng.anchor_append(sf.IDS[:5], sf.LENS[:5])
    m, counts = _model(eng)
    with pytest.raises(RuntimeError, match="keep=True"):
        m.rematch_arrays(arrays)
    m.sweep_arrays(arrays, batch_size=4)  # not a keeping sweep
    assert not [c for c in lib.log if c[0] == "keep"]
    with pytest.raises(RuntimeError, match="keep=True"):
        m.rematch_arrays(arrays)
    best, idx, ps = m.sweep_arrays(arrays, batch_size=4, keep=True, topk=2)
    eng.anchor_append(sf.IDS[:1], sf.LENS[:1])
    best2, idx2, ps2 = m.rematch_arrays(arrays)
    assert _rematches(lib) == [("rematch", 0, 8, 5, 0)] and best2.tobytes() == best.tobytes() and ps2 is None
    assert len(counts) == 3 and counts[2][0].tobytes() == counts[1][0].tobytes() and counts[2][1].tolist() == counts[1][1].tolist() == [0, 1, 1, 0, 1, 1, 1, 0]
    assert len(m._siamese_metric.calls) == 3 and m._siamese_metric.calls[2][1].tobytes() == best[:, 0].tobytes()
    with pytest.raises(RuntimeError, match="keep=True"):
        m.rematch_arrays(arrays, 0, 4)  # other rows than the kept sweep's
    # an engine without the new options keeps working as long as nothing new is asked of it
    m_old, counts_old = _model(_OldEngine())
    m_old.sweep_arrays(arrays, batch_size=4)
    assert len(counts_old) == 1
