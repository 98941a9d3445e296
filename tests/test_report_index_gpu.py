"""Per-anchor retrieval on the GPU (memvul_amd/retrieve.py, include/memvul_retrieve.h, csrc/report_topk.h).  The witness is the engine itself: anchor_set(V), then
match(U) in batches of max_batch gives probs[:, :, same_idx] — the bits every entry point of the engine produces for those pairs (match_topk.h: a pair's result
depends on the pair alone).  psame must be BYTE-equal to that matrix and query to its reference order.  There is no tolerance in this file."""
import ctypes as C
import os
import sys
import time
import warnings

import numpy as np
import pytest

from memvul_amd import retrieve, synth

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import report_index_kit as kit  # noqa: E402
from kept_index_kit import L2, WK, WK768, _engine_matrix, _same_bytes, bare_model  # noqa: E402

N_MAX, G_MAX, N_PLAN, G_PLAN = 1000, 257, 4099, 7


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


def _case(gu, P):
    """Once per embedding width: the fixture, the engine's matcher weight, and the engine's own probabilities of all pairs (shared, read-only)."""
    wk = WK if P == 512 else WK768
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = gu.engine_for(L2, wk, compute_dtype="precise", max_anchors=320, **({} if P == 512 else {"proj_dim": 768}))
    _, w = gu.weights_for(L2, wk)
    Wm = np.ascontiguousarray(w[synth.KEY_MATCH_W], np.float32)
    assert Wm.shape == (2, 3 * P)
    U, V, _ = kit.fixture(41 + P, N_PLAN if P == 512 else N_MAX, P, G_MAX, block_rows=64)
    probs = _engine_matrix(eng, U, V)
    for a in (U, V, probs):
        a.setflags(write=False)
    ps = probs[:, :, 0]
    with np.errstate(divide="ignore"):
        d = np.abs(np.log(ps / (1 - ps)))
    gu.record("report_index_fixture", P=P, delta_abs_median=float(np.median(d)), delta_abs_p99=float(np.percentile(d, 99)), p_min=float(ps.min()), p_max=float(ps.max()))
    assert np.median(d) > 0.3 and np.percentile(d, 1) < 0.5 and np.percentile(d, 99) < 16.0, "the fixture's P(same) must be neither all one half nor saturated"
    return dict(eng=eng, Wm=Wm, U=U, V=V, probs=probs)


@pytest.fixture(scope="module")
def c512(gu):
    return _case(gu, 512)


@pytest.fixture(scope="module")
def c768(gu):
    return _case(gu, 768)


def _index(c, same_idx, rows):
    ix = retrieve.ReportIndex(0, c["U"].shape[1], c["Wm"], same_idx)
    ix.add(np.ascontiguousarray(c["U"][:rows]))
    return ix


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_idx", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_psame_is_the_engines_matrix(gu, c512, N, same_idx):
    with _index(c512, same_idx, N) as ix:
        for G in (1, 3, 124, 257):
            got = ix.psame(np.ascontiguousarray(c512["V"][:G]))
            gu.record("report_index_psame", N=N, G=G, P=512, same_idx=same_idx, kernel_ms=ix.kernel_ms())
            _same_bytes(got, np.ascontiguousarray(c512["probs"][:N, :G, same_idx]), f"psame N={N} G={G}")


@pytest.mark.parametrize("N,G", [(65, 3), (1000, 124), (257, 257)])
def test_psame_at_768_features(gu, c768, N, G):
    for same_idx in (0, 1):
        with _index(c768, same_idx, N) as ix:
            got = ix.psame(np.ascontiguousarray(c768["V"][:G]))
            gu.record("report_index_psame", N=N, G=G, P=768, same_idx=same_idx, kernel_ms=ix.kernel_ms())
            _same_bytes(got, np.ascontiguousarray(c768["probs"][:N, :G, same_idx]), f"psame P=768 N={N} G={G}")
            tp, tr = ix.query(np.ascontiguousarray(c768["V"][:G]), 10)
            want_p, want_r = kit.reference_topk(c768["probs"][:N, :G, same_idx], 10)
            assert np.array_equal(tr, want_r)
            _same_bytes(tp, want_p, "query P=768")


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 65, 257, 1000])
def test_query_is_the_reference_order_of_the_engines_matrix(gu, c512, N):
    for same_idx, G in ((0, 124), (1, 7)):
        with _index(c512, same_idx, N) as ix:
            v = np.ascontiguousarray(c512["V"][:G])
            for k in (1, 10, 64):  # (k > N at the small sizes: exhausted slots -1 / -1)
                tp, tr = ix.query(v, k)
                gu.record("report_index_query", N=N, G=G, k=k, kernel_ms=ix.kernel_ms(), merge_levels=kit.merge_levels(N, 256, 16))
                want_p, want_r = kit.reference_topk(c512["probs"][:N, :G, same_idx], k)
                assert np.array_equal(tr, want_r), (N, G, k)
                _same_bytes(tp, want_p, f"query N={N} G={G} k={k}")
                if k > N:
                    assert (tr[:, N:] == -1).all() and (tp[:, N:] == -1.0).all()


def test_duplicates_rank_in_row_order_and_a_nan_row_first(gu, c512):
    """The fixture's exact duplicate rows (0 = 64, 2 = 3, 63 = 64 overwritten ...) tie bit for bit: the lower row comes first; a row holding a NaN ranks above all."""
    U = np.array(c512["U"][:300])
    U[200, 170] = np.float32("nan")
    V = np.ascontiguousarray(c512["V"][:7])
    probs = _engine_matrix(c512["eng"], U, V)
    assert np.isnan(probs[200]).all() and not np.isnan(np.delete(probs, 200, 0)).any()
    with retrieve.ReportIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        _same_bytes(ix.psame(V), np.ascontiguousarray(probs[:, :, 0]), "psame with a NaN row")  # (the NaN's own bits too)
        tp, tr = ix.query(V, 64)
        want_p, want_r = kit.reference_topk(probs[:, :, 0], 64)
        assert (tr[:, 0] == 200).all() and np.isnan(tp[:, 0]).all()
        assert np.array_equal(tr, want_r)
        _same_bytes(tp, want_p, "query with a NaN row")
        # rows 2 and 3 are duplicates: wherever one is listed the other follows it directly, lower row first (k = 64 of 300 rows: some vector lists them)
        tp, tr = ix.query(V, 64, 0, 64)
        for g in range(7):
            at = tr[g].tolist().index(2)
            assert tr[g, at + 1] == 3 and tp[g, at] == tp[g, at + 1]


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_no_plan_changes_a_byte(gu, c512):
    v = np.ascontiguousarray(c512["V"][:G_PLAN])
    want_p, want_r = kit.reference_topk(c512["probs"][:N_PLAN, :G_PLAN, 0], 10)
    assert kit.merge_levels(N_PLAN, 64, 2) >= 6
    with _index(c512, 0, N_PLAN) as ix:
        for plan in ((0, 0, 0), (64, 2, 1), (256, 3, 5), (64, 16, 7), (128, 5, 2), (512, 2, 3)):
            ix.test_plan(*plan)
            tp, tr = ix.query(v, 10)
            gu.record("report_index_plan", plan=list(plan), kernel_ms=ix.kernel_ms(), merge_levels=kit.merge_levels(N_PLAN, plan[0] or 256, plan[1] or 16))
            assert np.array_equal(tr, want_r), plan
            _same_bytes(tp, want_p, f"plan {plan}")
            _same_bytes(ix.psame(v, 1000, 300), np.ascontiguousarray(c512["probs"][1000:1300, :G_PLAN, 0]), f"psame under plan {plan}")


def test_a_grid_of_more_than_one_slice(gu, c512):
    """65 537 rows in blocks of 64 are 1 025 row blocks: the score kernel's grid has a second, ragged z-slice (RT_GRID_Y = 1024), and the one row in it is the one
    that differs.  The witness: the engine's values for the two kinds of row."""
    rows = 65537
    U = np.zeros((rows, 512), np.float32)
    U[rows - 1] = c512["U"][7]
    V = np.ascontiguousarray(np.stack([np.zeros(512, np.float32), c512["V"][0]]))
    two = _engine_matrix(c512["eng"], np.ascontiguousarray(U[[0, rows - 1]]), V)[:, :, 0]
    ps = np.repeat(two[:1], rows, 0)
    ps[rows - 1] = two[1]
    with retrieve.ReportIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        for plan in ((64, 16, 0), (0, 0, 0)):
            ix.test_plan(*plan)
            tp, tr = ix.query(V, 64)
            want_p, want_r = kit.reference_topk(ps, 64)
            assert np.array_equal(tr, want_r), plan
            _same_bytes(tp, want_p, f"two z-slices, plan {plan}")
            _same_bytes(ix.psame(V, rows - 100, 100), np.ascontiguousarray(ps[rows - 100:]), f"psame, plan {plan}")
            tp, tr = ix.query(V, 5, rows - 3, 3)
            assert sorted(tr[0, :3].tolist()) == [rows - 3, rows - 2, rows - 1] and (tr[:, 3:] == -1).all()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_sub_ranges_and_the_way_the_rows_arrived(gu, c512):
    v = np.ascontiguousarray(c512["V"][:G_PLAN])
    ps = c512["probs"][:N_PLAN, :G_PLAN, 0]
    with _index(c512, 0, N_PLAN) as ix, retrieve.ReportIndex(0, 512, c512["Wm"], 0) as parts:
        whole = ix.query(v, 10)
        for first, count in ((0, 256), (256, 512), (512, 3587), (1, 255), (100, 1), (255, 2), (257, 3000), (4098, 1), (4099, 0), (7, 0)):
            tp, tr = ix.query(v, 10, first, count)
            want_p, want_r = kit.reference_topk(ps[first:first + count], 10, first=first)
            assert np.array_equal(tr, want_r), (first, count)
            _same_bytes(tp, want_p, f"rows [{first}, +{count})")
            _same_bytes(ix.psame(v, first, count), np.ascontiguousarray(ps[first:first + count]), f"psame rows [{first}, +{count})")
        for a, b in ((0, 1000), (1000, 1001), (1001, N_PLAN)):
            parts.add(np.ascontiguousarray(c512["U"][a:b]))
        assert len(parts) == N_PLAN
        got = parts.query(v, 10)
        _same_bytes(got[0], whole[0], "three adds, p")
        _same_bytes(got[1], whole[1], "three adds, rows")
        parts.reset()
        assert len(parts) == 0
        tp, tr = parts.query(v, 3)
        assert (tr == -1).all() and (tp == -1.0).all()
        parts.add(np.ascontiguousarray(c512["U"][:N_PLAN]))
        got = parts.query(v, 10)
        _same_bytes(got[0], whole[0], "reset then add, p")
        _same_bytes(got[1], whole[1], "reset then add, rows")


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_query_vectors_do_not_see_each_other(gu, c512):
    G = 124
    v = np.ascontiguousarray(c512["V"][:G])
    with _index(c512, 0, N_MAX) as ix:
        tp, tr = ix.query(v, 10)
        a, b = ix.query(np.ascontiguousarray(v[:3]), 10), ix.query(np.ascontiguousarray(v[3:]), 10)
        _same_bytes(np.concatenate([a[0], b[0]]), tp, "stacked p")
        _same_bytes(np.concatenate([a[1], b[1]]), tr, "stacked rows")
        _same_bytes(tr[3], tr[1], "duplicate query vectors (3 = 1), rows")
        _same_bytes(tp[3], tp[1], "duplicate query vectors (3 = 1), p")


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_from_a_kept_sweep(gu, c512):
    eng = c512["eng"]
    dims, _ = gu.weights_for(L2, WK)
    n = 200
    ids, lens = synth.make_ids(n, 64, dims.vocab_size, seed=synth.SEED + 77, ragged=True, min_len=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng.anchor_reset()
        eng.anchor_append(*synth.make_ids(5, 64, dims.vocab_size, seed=synth.SEED + 78, ragged=True, min_len=16))
        eng.bucketed_sweep(ids, lens, 64, keep=True)
        with retrieve.ReportIndex.from_sweep(eng, c512["Wm"], 0, chunk=64) as ix:
            assert len(ix) == n
            for more in (0, 2):
                if more:
                    eng.anchor_append(*synth.make_ids(more, 64, dims.vocab_size, seed=synth.SEED + 79, ragged=True, min_len=16))
                ps = eng.rematch_sweep(with_probs=True)[2]
                tp, tr = ix.query(eng.anchor_get(), 10)
                want_p, want_r = kit.reference_topk(ps, 10)
                assert tp.shape == (5 + more, 10) and np.array_equal(tr, want_r)
                _same_bytes(tp, want_p, f"from_sweep, {5 + more} anchors")
        # the same through ModelMemory.anchor_reports
        m = bare_model(eng, c512["Wm"], 7)
        arrays = {"type": "test", "ids": ids, "lens": lens, "same": np.zeros(n, bool), "urls": [f"https://example.invalid/issues/{i}" for i in range(n)]}
        _, _, ps = m.sweep_arrays(arrays, batch_size=64, with_probs=True, keep=True)
        out = m.anchor_reports(arrays, 10)
        want_p, want_r = kit.reference_topk(ps, 10)
        assert [e["anchor"] for e in out] == m._golden_labels
        for g, e in enumerate(out):
            assert [r["row"] for r in e["reports"]] == want_r[g].tolist() and [r["Issue_Url"] for r in e["reports"]] == [arrays["urls"][r] for r in want_r[g]]
            assert np.array([r["prob"] for r in e["reports"]], np.float32).tobytes() == want_p[g].tobytes()
        m._kept.drop()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_strictness(gu, c512):
    lib = retrieve.load_library()
    h = C.c_void_p()
    for args, words in (((0, 500, 0), b"512"), ((0, 512, 2), b"same_idx"), ((4096, 512, 0), b"device")):
        assert lib.mvr_create(args[0], args[1], c512["Wm"].ctypes.data_as(C.c_void_p), args[2], C.byref(h)) != 0 and not h.value
        assert words in lib.mvr_last_error(None), lib.mvr_last_error(None)
    rows = 65537
    with retrieve.ReportIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(np.zeros((rows, 512), np.float32))
        hh = ix._h
        v = np.zeros((4097, 512), np.float32)
        p, r = np.full((4097 * 64,), 7.0, np.float32), np.full((4097 * 64,), 7, np.int64)
        big = np.full((16,), 7.0, np.float32)
        vp, pp, rp = (a.ctypes.data_as(C.c_void_p) for a in (v, p, r))

        def refused(rc, words):
            msg = lib.mvr_last_error(hh)
            assert rc != 0 and words in msg, (rc, msg)
            assert (p == 7.0).all() and (r == 7).all() and (big == 7.0).all()

        refused(lib.mvr_query(hh, vp, 3, 0, 0, rows, pp, rp), b"k = 0")
        refused(lib.mvr_query(hh, vp, 3, 65, 0, rows, pp, rp), b"k = 65")
        refused(lib.mvr_query(hh, vp, 0, 3, 0, rows, pp, rp), b"Q = 0")
        refused(lib.mvr_query(hh, vp, 4097, 3, 0, rows, pp, rp), b"Q = 4097")
        refused(lib.mvr_query(hh, vp, 3, 3, -1, 5, pp, rp), b"rows [")
        refused(lib.mvr_query(hh, vp, 3, 3, 1, rows, pp, rp), b"rows [")
        refused(lib.mvr_query(hh, vp, 3, 3, rows + 1, 0, pp, rp), b"rows [")
        refused(lib.mvr_query(hh, None, 3, 3, 0, rows, pp, rp), b"NULL")
        refused(lib.mvr_psame(hh, vp, 4096, 0, rows, big.ctypes.data_as(C.c_void_p)), b"2^28")
        refused(lib.mvr_psame(hh, vp, 0, 0, 5, big.ctypes.data_as(C.c_void_p)), b"Q = 0")
        refused(lib.mvr_psame(hh, vp, 3, 5, rows, big.ctypes.data_as(C.c_void_p)), b"rows [")
        refused(lib.mvr_add(hh, vp, 2 ** 31), b"2^31 - 2")  # (refused before the buffer is looked at)
        refused(lib.mvr_add(hh, vp, -1), b"n = -1")
        for plan in ((100, 0, 0), (1024, 0, 0), (64, 1, 0), (64, 17, 0), (64, 2, -1), (64, 2, 4097)):
            refused(lib.mvr_test_plan(hh, *plan), b"= ")
        assert len(ix) == rows
        ms = C.c_float(7.0)
        refused(lib.mvr_kernel_ms(hh, None), b"NULL")
        # and the index still answers: zero rows against zero vectors are all alike, the lowest rows win
        t0 = time.perf_counter()
        tp, tr = ix.query(np.zeros((2, 512), np.float32), 3)
        gu.record("report_index_query", N=rows, G=2, k=3, kernel_ms=ix.kernel_ms(), wall_ms=(time.perf_counter() - t0) * 1e3, merge_levels=kit.merge_levels(rows, 256, 16))
        assert tr.tolist() == [[0, 1, 2], [0, 1, 2]] and (tp == 0.5).all()
        assert lib.mvr_kernel_ms(hh, C.byref(ms)) == 0 and 0 < ms.value < 1e4
