"""Per-anchor claims on the GPU (memvul_amd/claims.py, include/memvul_claims.h, csrc/claim_sweep.h).  The witness is the engine itself: anchor_set(V), then match(U)
gives probs[:, :, same_idx] — the bits every entry point of the engine produces for those pairs — and, in one test, ReportIndex.psame.  counts must EQUAL
(P >= t) split by class over that matrix, and select its offsets, rows and the bytes of p.  The thresholds are taken from the matrix itself (claims_kit.
matrix_thresholds: entries, and their neighbours one fp32 step up and down), so a single differing bit of P(same) moves a count.  There is no tolerance in this file.

Every test first asserts, on the reference alone, that its thresholds bite: some (vector, threshold) claims nothing, some claims every non-NaN row, and the pooled
claimed share lies between 5 % and 95 %."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import claims, retrieve, synth

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import claims_kit as kit  # noqa: E402
from kept_index_kit import L2, WK, WK768, _engine_matrix, _same_bytes, bare_model  # noqa: E402

N_PLAN, N_MAX, Q_MAX, Q_768, Q_PLAN = 4099, 1000, 33, 124, 7


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
    U, V, _ = kit.rkit.fixture(43 + P, N_PLAN if P == 512 else N_MAX, P, Q_MAX if P == 512 else Q_768, block_rows=64)
    probs = _engine_matrix(eng, U, V)
    cls = (np.random.default_rng(3).random(len(U)) < 0.3).astype(np.uint8)
    for a in (U, V, probs, cls):
        a.setflags(write=False)
    return dict(eng=eng, Wm=Wm, U=U, V=V, probs=probs, cls=cls)


@pytest.fixture(scope="module")
def c512(gu):
    return _case(gu, 512)


@pytest.fixture(scope="module")
def c768(gu):
    return _case(gu, 768)


def _index(c, same_idx, rows, cls=None):
    ix = claims.ClaimIndex(0, c["U"].shape[1], c["Wm"], same_idx)
    ix.add(np.ascontiguousarray(c["U"][:rows]))
    if cls is not None:
        ix.set_classes(np.ascontiguousarray(cls[:rows]))
    return ix


class _Bite:
    """The fixture condition, gathered over the (vector, threshold) pairs a test compares and asserted on the reference alone."""

    def __init__(self):
        self.none = self.every = False
        self.claimed = self.pairs = 0

    def see(self, ps, th):
        """ps [N, Q]; th [T] (every vector meets every threshold) or [Q, K] (vector q meets th[q])."""
        th = np.asarray(th, np.float32)
        with np.errstate(invalid="ignore"):
            hit = ps[:, :, None] >= (th[None, None, :] if th.ndim == 1 else th[None, :, :])  # [N, Q, T]
        n = hit.sum(0)
        live = (~np.isnan(ps)).sum(0)[:, None]
        self.none = self.none or bool((n == 0).any())
        self.every = self.every or bool(((n == live) & (live > 0)).any())
        self.claimed += int(n.sum())
        self.pairs += int(hit.size)

    def check(self):
        share = self.claimed / max(self.pairs, 1)
        assert self.none and self.every and 0.05 < share < 0.95, (self.none, self.every, share)
        return share


def _pool(th: np.ndarray, T: int) -> np.ndarray:
    """T thresholds out of the per-vector ones [Q, 15], in no particular order, duplicates where there are fewer than T: 0.0, 1.0, 1.0's neighbour and the first
    vector's four percentile values always among them from T = 40 on; T = 1 takes a median."""
    if T == 1:
        return np.ascontiguousarray(th[0, 1:2])
    flat = np.concatenate([th[0, 12:15], th[:, :12].reshape(-1)])
    return np.ascontiguousarray(flat[np.arange(T) % len(flat)])


def _classes(kind, cls, N):
    if kind == "zeros":
        return np.zeros(N, np.uint8), lambda ix: None
    if kind == "alternating":
        c = (np.arange(N) % 2).astype(np.uint8)
        return c, lambda ix: ix.set_classes(c)
    # two overlapping calls: the second overwrites the tail of the first
    want = np.array(cls[:N])
    a = N * 2 // 3
    b = N // 3

    def two(ix):
        ix.set_classes(np.ascontiguousarray(1 - want[:a]))
        ix.set_classes(np.ascontiguousarray(want[b:]), b)
        ix.set_classes(np.ascontiguousarray(want[:b]))
    return want, two


# ---- 1: counts ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_idx", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_are_the_matrix_met_with_the_rule(gu, c512, N, same_idx):
    bite = _Bite()
    cases = []
    for Q in (1, 15, 16, 17, 33):
        ps = c512["probs"][:N, :Q, same_idx]
        th = kit.matrix_thresholds(ps)
        for T in (1, 40, 64):
            pool = _pool(th, T)
            bite.see(ps, pool)
            cases.append((Q, ps, pool))
    bite.check()
    with _index(c512, same_idx, N) as ix:
        for kind in ("zeros", "alternating", "overlapping"):
            cls, set_them = _classes(kind, c512["cls"], N)
            set_them(ix)
            for Q, ps, pool in cases:
                got = ix.counts(np.ascontiguousarray(c512["V"][:Q]), pool)
                if Q == 33 and kind == "zeros":  # (one figure per size and T: the records are read by people)
                    gu.record("claims_counts", N=N, Q=Q, T=len(pool), P=512, same_idx=same_idx, kernel_ms=ix.kernel_ms())
                want = kit.reference_counts(ps, cls, pool)
                assert got.dtype == np.int64 and np.array_equal(got, want), (N, Q, len(pool), kind, np.argwhere(got != want)[:3].tolist())
                if kind == "zeros":
                    assert (got[:, :, 1] == 0).all()


@pytest.mark.parametrize("N,Q", [(65, 3), (1000, 124)])
def test_counts_and_select_at_768_features(gu, c768, N, Q):
    for same_idx in (0, 1):
        ps = c768["probs"][:N, :Q, same_idx]
        th = kit.matrix_thresholds(ps)
        bite = _Bite()
        bite.see(ps, _pool(th, 40))
        bite.see(ps, th[:, [0, 1, 5, 13]])
        bite.check()
        v = np.ascontiguousarray(c768["V"][:Q])
        with _index(c768, same_idx, N, c768["cls"]) as ix:
            got = ix.counts(v, _pool(th, 40))
            gu.record("claims_counts", N=N, Q=Q, T=40, P=768, same_idx=same_idx, classes="random", kernel_ms=ix.kernel_ms())
            assert np.array_equal(got, kit.reference_counts(ps, c768["cls"][:N], _pool(th, 40)))
            for col in (0, 1, 5, 13):
                off, rows, p = ix.select(v, np.ascontiguousarray(th[:, col]), order="row")
                want = kit.reference_select(ps, th[:, col])
                assert np.array_equal(off, want[0]) and np.array_equal(rows, want[1]), (N, Q, col)
                _same_bytes(p, want[2], f"select P=768 N={N} Q={Q} column {col}")


# ---- 2: select ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_idx", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_select_is_the_matrix_met_with_the_rule(gu, c512, N, same_idx):
    bite = _Bite()
    for Q in (1, 15, 16, 17, 33):
        bite.see(c512["probs"][:N, :Q, same_idx], kit.matrix_thresholds(c512["probs"][:N, :Q, same_idx]))
    bite.check()
    short = 0
    with _index(c512, same_idx, N) as ix, retrieve.ReportIndex(0, 512, c512["Wm"], same_idx) as rx:
        rx.add(np.ascontiguousarray(c512["U"][:N]))
        for Q in (1, 15, 16, 17, 33):
            ps = c512["probs"][:N, :Q, same_idx]
            th = kit.matrix_thresholds(ps)
            v = np.ascontiguousarray(c512["V"][:Q])
            top_p, top_r = rx.query(v, 64)
            for k in range(15):  # vector q meets its threshold (k + q) mod 15: every vector meets every one of its own
                thres = np.ascontiguousarray(th[np.arange(Q), (k + np.arange(Q)) % 15])
                off, rows, p = ix.select(v, thres, order="row")
                if Q == 33 and k == 0:
                    gu.record("claims_select", N=N, Q=Q, P=512, same_idx=same_idx, pairs=int(off[-1]), kernel_ms=ix.kernel_ms())
                want = kit.reference_select(ps, thres)
                assert off.dtype == rows.dtype == np.int64 and np.array_equal(off, want[0]) and np.array_equal(rows, want[1]), (N, Q, k)
                _same_bytes(p, want[2], f"select N={N} Q={Q} round {k}")
                if k % 5 == 0:  # retrieval's order, and retrieval's own leading entries where a vector claims at most 64 rows
                    off2, rows2, p2 = ix.select(v, thres, order="prob")
                    want_r, want_p = kit.by_prob(*want)
                    assert np.array_equal(off2, off) and np.array_equal(rows2, want_r)
                    _same_bytes(p2, want_p, "order = prob")
                    for q in range(Q):
                        n = int(off[q + 1] - off[q])
                        if n <= 64:
                            short += n > 0
                            assert np.array_equal(rows2[off[q]:off[q + 1]], top_r[q, :n]), (N, Q, k, q)
                            _same_bytes(p2[off[q]:off[q + 1]], np.ascontiguousarray(top_p[q, :n]), "the leading entries of query(k = 64)")
    assert short > 0


# ---- 3: a NaN row ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_nan_row_is_never_claimed_and_never_counted(gu, c512):
    U = np.array(c512["U"][:300])
    U[200, 170] = np.float32("nan")
    V = np.ascontiguousarray(c512["V"][:Q_PLAN])
    probs = _engine_matrix(c512["eng"], U, V)
    assert np.isnan(probs[200]).all() and not np.isnan(np.delete(probs, 200, 0)).any()
    ps = probs[:, :, 0]
    th = kit.matrix_thresholds(ps)
    bite = _Bite()
    bite.see(ps, th)
    bite.check()
    cls = np.ones(300, np.uint8)
    with claims.ClaimIndex(0, 512, c512["Wm"], 0) as ix, retrieve.ReportIndex(0, 512, c512["Wm"], 0) as rx:
        ix.add(U)
        ix.set_classes(cls)
        rx.add(U)
        _same_bytes(rx.psame(V), np.ascontiguousarray(ps), "the witness: psame with a NaN row")
        pool = np.ascontiguousarray(np.concatenate([[0.0, -1.0], th[0]]).astype(np.float32))
        got = ix.counts(V, pool)
        assert np.array_equal(got, kit.reference_counts(ps, cls, pool)) and (got[:, 0].sum(1) == 299).all() and (got[:, 1].sum(1) == 299).all()
        for col in range(15):
            off, rows, p = ix.select(V, np.ascontiguousarray(th[:, col]), order="row")
            want = kit.reference_select(ps, th[:, col])
            assert np.array_equal(off, want[0]) and np.array_equal(rows, want[1]) and 200 not in rows
            _same_bytes(p, want[2], "select with a NaN row")
        off, rows, p = ix.select(V, 0.0, order="row")  # everything but the NaN row: its neighbours are where they belong
        assert np.array_equal(np.diff(off), np.full(Q_PLAN, 299)) and np.array_equal(rows[:299], np.delete(np.arange(300), 200))
        _same_bytes(p, np.ascontiguousarray(np.delete(ps, 200, 0).T).reshape(-1), "threshold 0 with a NaN row")


# ---- 4: the plan ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_no_plan_changes_a_byte(gu, c512):
    v = np.ascontiguousarray(c512["V"][:Q_PLAN])
    ps = c512["probs"][:N_PLAN, :Q_PLAN, 0]
    th = kit.matrix_thresholds(ps)
    pool = _pool(th, 40)
    bite = _Bite()
    bite.see(ps, pool)
    bite.see(ps, th[:, [1, 2, 12]])
    bite.check()
    want_c = kit.reference_counts(ps, c512["cls"], pool)
    want_s = {col: kit.reference_select(ps, th[:, col]) for col in (1, 2, 12)}
    with _index(c512, 0, N_PLAN, c512["cls"]) as ix:
        for block_rows in (0, 64, 128, 256, 512):
            for group in (0, 1, 5):
                ix.test_plan(block_rows, group)
                got = ix.counts(v, pool)
                gu.record("claims_plan", plan=[block_rows, group], kernel_ms=ix.kernel_ms())
                assert np.array_equal(got, want_c), (block_rows, group)
                assert np.array_equal(ix.counts(v, pool, 1000, 300), kit.reference_counts(ps[1000:1300], c512["cls"][1000:1300], pool)), (block_rows, group)
                for col, want in want_s.items():
                    off, rows, p = ix.select(v, np.ascontiguousarray(th[:, col]), order="row")
                    assert np.array_equal(off, want[0]) and np.array_equal(rows, want[1]), (block_rows, group, col)
                    _same_bytes(p, want[2], f"plan ({block_rows}, {group}) column {col}")


def test_two_grid_slices_and_the_pair_limit(gu, c512):
    """65 537 rows in blocks of 64 are 1 025 row blocks: the score kernel's grid has a second, ragged z-slice (CL_GRID_Y = 1024), and the one row in it is the one
    that differs.  The same rows against 4 096 vectors at threshold 0 are 2^28 + 4 096 pairs, just over MVC_MAX_PAIRS — the real limit on a real selection, no
    test hook: it is refused once the totals are known, with the total in the message and before anything is allocated for the pairs."""
    rows = 65537
    U = np.zeros((rows, 512), np.float32)
    U[rows - 1] = c512["U"][7]
    V = np.ascontiguousarray(np.stack([np.zeros(512, np.float32), c512["V"][0]]))
    two = _engine_matrix(c512["eng"], np.ascontiguousarray(U[[0, rows - 1]]), V)[:, :, 0]
    ps = np.repeat(two[:1], rows, 0)
    ps[rows - 1] = two[1]
    assert two[0, 0] == 0.5 and len(set(two.reshape(-1).tolist())) == 4
    cls = np.zeros(rows, np.uint8)
    cls[[5, rows - 1]] = 1
    th = np.ascontiguousarray(np.sort(two.reshape(-1)))
    bite = _Bite()
    bite.see(ps, np.concatenate([th, [np.nextafter(th[-1], np.float32(2))]]).astype(np.float32))
    bite.check()
    with claims.ClaimIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        ix.set_classes(cls)
        for plan in ((64, 0), (0, 0)):
            ix.test_plan(*plan)
            pool = np.concatenate([th, [np.nextafter(th[-1], np.float32(2))]]).astype(np.float32)
            got = ix.counts(V, pool)
            gu.record("claims_counts", N=rows, Q=2, T=5, P=512, same_idx=0, classes="two", plan=list(plan), kernel_ms=ix.kernel_ms())
            assert np.array_equal(got, kit.reference_counts(ps, cls, pool)), plan
            assert np.array_equal(ix.counts(V, pool, rows - 3, 3), kit.reference_counts(ps[rows - 3:], cls[rows - 3:], pool))
            for t in th:
                off, r, p = ix.select(V, np.float32(t), order="row")
                want = kit.reference_select(ps, np.full(2, t, np.float32))
                assert np.array_equal(off, want[0]) and np.array_equal(r, want[1]), (plan, float(t))
                _same_bytes(p, want[2], f"two z-slices, plan {plan}")
        ix.test_plan(0, 0)
        lib, h = ix._lib, ix._h
        big = np.zeros((4096, 512), np.float32)
        off = np.full(4097, 7, np.int64)
        rc = lib.mvc_select(h, big.ctypes.data_as(C.c_void_p), 4096, np.zeros(4096, np.float32).ctypes.data_as(C.c_void_p), 0, rows, off.ctypes.data_as(C.c_void_p))
        msg = lib.mvc_last_error(h)
        gu.record("claims_select_refused", N=rows, Q=4096, kernel_ms=ix.kernel_ms())
        assert rc == -1 and str(rows * 4096).encode() in msg and b"2^28" in msg and (off == 7).all(), (rc, msg)
        assert lib.mvc_fetch(h, None, None) == claims.ERR_STATE  # nothing is held after the refusal
        off, r, p = ix.select(big[:2], 0.0, rows - 70, 70, order="row")  # and the index still answers
        assert off.tolist() == [0, 70, 140] and np.array_equal(r[:70], np.arange(rows - 70, rows)) and (p[:69] == 0.5).all()


# ---- 5: sub-ranges and the way the rows arrived ---------------------------------------------------------------------------------------------------------------------

def test_sub_ranges_and_the_way_the_rows_arrived(gu, c512):
    N = 257
    v = np.ascontiguousarray(c512["V"][:Q_PLAN])
    ps, cls = c512["probs"][:N, :Q_PLAN, 0], c512["cls"][:N]
    th = kit.matrix_thresholds(ps)
    pool = _pool(th, 40)
    bite = _Bite()
    bite.see(ps, pool)
    bite.see(ps, th[:, [1, 12]])
    bite.check()

    def compare(ix, what):
        for first, count in ((0, N), (1, N - 1), (63, 130), (64, 64), (N - 1, 1), (5, 0)):
            got = ix.counts(v, pool, first, count)
            assert np.array_equal(got, kit.reference_counts(ps[first:first + count], cls[first:first + count], pool)), (what, first, count)
            for col in (1, 12):
                off, rows, p = ix.select(v, np.ascontiguousarray(th[:, col]), first, count, order="row")
                want = kit.reference_select(ps[first:first + count], th[:, col], first)
                assert np.array_equal(off, want[0]) and np.array_equal(rows, want[1]), (what, first, count, col)
                _same_bytes(p, want[2], f"{what}: rows [{first}, +{count}) column {col}")

    with _index(c512, 0, N, c512["cls"]) as ix, claims.ClaimIndex(0, 512, c512["Wm"], 0) as parts:
        compare(ix, "one add")
        for a, b in ((0, 1), (1, 64), (64, N)):
            parts.add(np.ascontiguousarray(c512["U"][a:b]))
        assert len(parts) == N
        parts.set_classes(np.ascontiguousarray(cls))
        compare(parts, "adds of 1, 63 and the rest")
        parts.reset()
        assert len(parts) == 0
        assert (parts.counts(v, pool) == 0).all() and parts.select(v, 0.0)[0].tolist() == [0] * (Q_PLAN + 1)
        parts.add(np.ascontiguousarray(c512["U"][:N]))
        assert (parts.counts(v, pool)[:, :, 1] == 0).all()  # the classes went with the rows
        parts.set_classes(np.ascontiguousarray(cls))
        compare(parts, "reset then add")


# ---- 6: the vectors do not see each other -----------------------------------------------------------------------------------------------------------------------------

def test_the_vectors_do_not_see_each_other(gu, c512):
    Q = 33
    v = np.ascontiguousarray(c512["V"][:Q])
    ps = c512["probs"][:N_MAX, :Q, 0]
    th = kit.matrix_thresholds(ps)
    pool = _pool(th, 40)
    thres = np.ascontiguousarray(th[np.arange(Q), np.arange(Q) % 15])
    bite = _Bite()
    bite.see(ps, pool)
    bite.see(ps, th)
    bite.check()
    assert np.array_equal(v[3], v[1]) and np.array_equal(v[Q - 1], v[0])  # the fixture's duplicate vectors
    with _index(c512, 0, N_MAX, c512["cls"]) as ix:
        whole = ix.counts(v, pool)
        assert np.array_equal(whole, kit.reference_counts(ps, c512["cls"][:N_MAX], pool))
        assert np.array_equal(np.concatenate([ix.counts(np.ascontiguousarray(v[:3]), pool), ix.counts(np.ascontiguousarray(v[3:]), pool)]), whole)
        assert np.array_equal(whole[3], whole[1]) and np.array_equal(whole[Q - 1], whole[0])
        off, rows, p = ix.select(v, thres, order="row")
        for q in (0, 5, 16, Q - 1):  # alone, first, last, and twice: the same segment
            seg = (rows[off[q]:off[q + 1]], p[off[q]:off[q + 1]])
            for vv, tt, at in ((v[q:q + 1], thres[q:q + 1], 0), (np.concatenate([v[q:q + 1], v[:20]]), np.concatenate([thres[q:q + 1], thres[:20]]), 0),
                               (np.concatenate([v[:20], v[q:q + 1]]), np.concatenate([thres[:20], thres[q:q + 1]]), 20),
                               (np.concatenate([v[q:q + 1], v[q:q + 1]]), np.concatenate([thres[q:q + 1], thres[q:q + 1]]), 1)):
                o, r, pp = ix.select(np.ascontiguousarray(vv), np.ascontiguousarray(tt), order="row")
                assert np.array_equal(r[o[at]:o[at + 1]], seg[0]), q
                _same_bytes(pp[o[at]:o[at + 1]], seg[1], f"vector {q} at place {at}")


# ---- 7: the held selection --------------------------------------------------------------------------------------------------------------------------------------------

def test_the_held_selection(gu, c512):
    """The rule of include/memvul_claims.h: mvc_fetch follows a successful mvc_select as often as asked; mvc_count, mvc_kernel_ms and mvc_last_error leave the
    selection alone; every other call on the index drops it."""
    N = 257
    v = np.ascontiguousarray(c512["V"][:Q_PLAN])
    ps = c512["probs"][:N, :Q_PLAN, 0]
    th = kit.matrix_thresholds(ps)
    bite = _Bite()
    bite.see(ps, th)
    bite.check()
    want = kit.reference_select(ps, th[:, 1])
    with _index(c512, 0, N) as ix:
        lib, h = ix._lib, ix._h
        rows, p = np.full(N * Q_PLAN, 7, np.int64), np.full(N * Q_PLAN, 7.0, np.float32)

        def no_selection():
            rc = lib.mvc_fetch(h, rows.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p))
            assert rc == claims.ERR_STATE and b"no selection is held" in lib.mvc_last_error(h) and (rows == 7).all() and (p == 7.0).all()
            with pytest.raises(RuntimeError, match="no selection is held"):
                ix.fetch(1)

        no_selection()  # nothing selected yet
        off, r, pp = ix.select(v, np.ascontiguousarray(th[:, 1]), order="row")
        assert len(ix) == N and ix.kernel_ms() > 0
        for _ in range(2):  # as often as asked, and after the calls that leave it alone
            r2, p2 = ix.fetch(int(off[-1]))
            assert np.array_equal(r2, want[1]) and p2.tobytes() == want[2].tobytes()
        ix.counts(v, np.ascontiguousarray(th[0]))
        no_selection()  # a counts call in between
        for drop in (lambda: ix.reset(), lambda: ix.add(np.ascontiguousarray(c512["U"][:N])), lambda: ix.set_classes(np.zeros(3, np.uint8)), lambda: ix.test_plan(0, 0)):
            if len(ix):
                ix.select(v, np.ascontiguousarray(th[:, 1]))
            drop()
            no_selection()
        off, r, pp = ix.select(v, np.ascontiguousarray(th[:, 1]), N, 0)  # an empty range: an empty selection is held
        assert off.tolist() == [0] * (Q_PLAN + 1) and len(r) == 0 and lib.mvc_fetch(h, None, None) == 0
        assert lib.mvc_select(h, v.ctypes.data_as(C.c_void_p), 0, th.ctypes.data_as(C.c_void_p), 0, N, off.ctypes.data_as(C.c_void_p)) != 0
        no_selection()  # a refused select holds nothing either


# ---- 8: strictness ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_strictness(gu, c512):
    lib = claims.load_library()
    h = C.c_void_p()
    for args, words in (((0, 500, 0), b"512"), ((0, 512, 2), b"same_idx"), ((4096, 512, 0), b"device")):
        assert lib.mvc_create(args[0], args[1], c512["Wm"].ctypes.data_as(C.c_void_p), args[2], C.byref(h)) != 0 and not h.value
        assert words in lib.mvc_last_error(None), lib.mvc_last_error(None)
    assert lib.mvc_create(0, 512, None, 0, C.byref(h)) != 0 and b"NULL" in lib.mvc_last_error(None)
    N = 300
    with _index(c512, 0, N, c512["cls"]) as ix:
        hh = ix._h
        v = np.zeros((4097, 512), np.float32)
        v[:Q_PLAN] = c512["V"][:Q_PLAN]
        th = np.full(4097, 0.5, np.float32)
        nan_th = th.copy()
        nan_th[2] = np.float32("nan")
        inf_th = th.copy()
        inf_th[0] = np.float32("inf")
        counts, off = np.full(4097 * 64 * 2, 7, np.int64), np.full(4098, 7, np.int64)
        cls2 = np.array([0, 1, 2], np.uint8)
        vp, tp, cp, op = (a.ctypes.data_as(C.c_void_p) for a in (v, th, counts, off))
        ps = c512["probs"][:N, :Q_PLAN, 0]
        pool = np.ascontiguousarray(kit.matrix_thresholds(ps)[0])
        bite = _Bite()
        bite.see(ps, pool)
        bite.check()
        before = ix.counts(np.ascontiguousarray(v[:Q_PLAN]), pool)
        assert np.array_equal(before, kit.reference_counts(ps, c512["cls"][:N], pool))

        def refused(rc, words):
            msg = lib.mvc_last_error(hh)
            assert rc != 0 and words in msg, (rc, msg)
            assert (counts == 7).all() and (off == 7).all()

        refused(lib.mvc_counts(hh, vp, 0, tp, 3, 0, N, cp), b"Q = 0")
        refused(lib.mvc_counts(hh, vp, 4097, tp, 3, 0, N, cp), b"Q = 4097")
        refused(lib.mvc_counts(hh, vp, 3, tp, 0, 0, N, cp), b"T = 0")
        refused(lib.mvc_counts(hh, vp, 3, tp, 65, 0, N, cp), b"T = 65")
        refused(lib.mvc_counts(hh, vp, 3, nan_th.ctypes.data_as(C.c_void_p), 3, 0, N, cp), b"thres[2] is not finite")
        refused(lib.mvc_counts(hh, vp, 3, inf_th.ctypes.data_as(C.c_void_p), 3, 0, N, cp), b"thres[0] is not finite")
        refused(lib.mvc_counts(hh, vp, 3, tp, 3, -1, 5, cp), b"rows [")
        refused(lib.mvc_counts(hh, vp, 3, tp, 3, 1, N, cp), b"rows [")
        refused(lib.mvc_counts(hh, vp, 3, tp, 3, N + 1, 0, cp), b"rows [")
        refused(lib.mvc_counts(hh, None, 3, tp, 3, 0, N, cp), b"NULL")
        refused(lib.mvc_counts(hh, vp, 3, None, 3, 0, N, cp), b"NULL")
        refused(lib.mvc_counts(hh, vp, 3, tp, 3, 0, N, None), b"NULL")
        refused(lib.mvc_select(hh, vp, 0, tp, 0, N, op), b"Q = 0")
        refused(lib.mvc_select(hh, vp, 4097, tp, 0, N, op), b"Q = 4097")
        refused(lib.mvc_select(hh, vp, 3, nan_th.ctypes.data_as(C.c_void_p), 0, N, op), b"thres[2] is not finite")
        refused(lib.mvc_select(hh, vp, 3, tp, 2, N - 1, op), b"rows [")
        refused(lib.mvc_select(hh, None, 3, tp, 0, N, op), b"NULL")
        refused(lib.mvc_select(hh, vp, 3, None, 0, N, op), b"NULL")
        refused(lib.mvc_select(hh, vp, 3, tp, 0, N, None), b"NULL")
        refused(lib.mvc_set_classes(hh, cls2.ctypes.data_as(C.c_void_p), 0, 3), b"cls[2] = 2")
        refused(lib.mvc_set_classes(hh, cls2.ctypes.data_as(C.c_void_p), N - 2, 3), b"rows [")
        refused(lib.mvc_set_classes(hh, None, 0, 3), b"NULL")
        refused(lib.mvc_add(hh, vp, 2 ** 31), b"2^31 - 2")  # (refused before the buffer is looked at)
        refused(lib.mvc_add(hh, vp, -1), b"n = -1")
        refused(lib.mvc_add(hh, None, 3), b"NULL")
        for plan in ((100, 0), (1024, 0), (64, -1), (64, 4097)):
            refused(lib.mvc_test_plan(hh, *plan), b"= ")
        refused(lib.mvc_kernel_ms(hh, None), b"NULL")
        assert lib.mvc_counts(None, vp, 3, tp, 3, 0, N, cp) != 0 and b"index is NULL" in lib.mvc_last_error(None) and (counts == 7).all()
        # a refused class value changed nothing, and the index still answers as before
        assert len(ix) == N and np.array_equal(ix.counts(np.ascontiguousarray(v[:Q_PLAN]), pool), before)
        ms = C.c_float(7.0)
        assert lib.mvc_kernel_ms(hh, C.byref(ms)) == 0 and 0 < ms.value < 1e4


# ---- 9: end to end ----------------------------------------------------------------------------------------------------------------------------------------------------

def _best_by_the_references_rule(col, same, grid64):
    """custom_metric.py:35-52 restated: Python floats of the fp32 scores against the float64 grid, best F1, `>=` — the last threshold wins a tie."""
    best_f1, best = 0, None
    for t in grid64.tolist():
        pred = col.astype(np.float64) >= t
        TP, FP, FN = int((pred & same).sum()), int((pred & ~same).sum()), int((~pred & same).sum())
        pd = TP / (TP + FN) if TP + FN else 0
        prec = TP / (TP + FP) if TP + FP else 0
        f1 = 2 * pd * prec / (pd + prec) if pd + prec else 0
        if f1 >= best_f1:
            best_f1, best = f1, t
    return best


def test_end_to_end_from_a_kept_sweep(gu, c512):
    eng = c512["eng"]
    dims, _ = gu.weights_for(L2, WK)
    n = 200
    ids, lens = synth.make_ids(n, 64, dims.vocab_size, seed=synth.SEED + 77, ragged=True, min_len=3)
    same = np.random.default_rng(9).random(n) < 0.3
    grid64 = np.arange(0.5, 0.9, 0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng.anchor_reset()
        eng.anchor_append(*synth.make_ids(5, 64, dims.vocab_size, seed=synth.SEED + 78, ragged=True, min_len=16))
        m = bare_model(eng, c512["Wm"], 5)
        arrays = {"type": "test", "ids": ids, "lens": lens, "same": same, "urls": [f"https://example.invalid/issues/{i}" for i in range(n)]}
        m.sweep_arrays(arrays, batch_size=64, with_probs=True, keep=True)
        for more in (0, 2):
            if more:  # the bank is edited, the corpus is not encoded again and the index is not refilled
                eng.anchor_append(*synth.make_ids(more, 64, dims.vocab_size, seed=synth.SEED + 79, ragged=True, min_len=16))
                m._golden_labels = [f"CWE-{i}" for i in range(5 + more)]
            index = m._kept.indexes["claims"]
            ps = m.rematch_arrays(arrays, with_probs=True)[2]
            assert ps.dtype == np.float32 and ps.shape == (n, 5 + more)
            mid = float(np.median(ps))
            bite = _Bite()
            bite.see(ps, np.array([mid, 0.0, 1.5], np.float32))
            share = bite.check()
            gu.record("claims_end_to_end", anchors=5 + more, share_at_half=float((ps >= 0.5).mean()), share_at_median=share)
            for thres, grid in ((0.5, None), (mid, "reference"), ([mid] * (4 + more) + [0.0], None)):
                out = m.anchor_claims(arrays, thres, grid=grid)
                assert more == 0 or m._kept.indexes["claims"] is index
                assert [e["anchor"] for e in out] == m._golden_labels
                for g, e in enumerate(out):
                    t = thres[g] if isinstance(thres, list) else thres
                    rows = [int(i) for i in np.flatnonzero(ps[:, g].astype(np.float64) >= t)]
                    rows.sort(key=lambda i: (-float(ps[i, g]), i))
                    assert e["thres"] == t and e["claimed"] == len(rows) and e["positives"] == int(same[rows].sum())
                    assert [r["row"] for r in e["reports"]] == rows and [r["Issue_Url"] for r in e["reports"]] == [arrays["urls"][r] for r in rows]
                    assert np.array([r["prob"] for r in e["reports"]], np.float32).tobytes() == ps[rows, g].tobytes()
                    if grid is not None:
                        assert [x["thres"] for x in e["grid"]] == grid64.tolist()
                        for x in e["grid"]:
                            pred = ps[:, g].astype(np.float64) >= x["thres"]
                            assert (x["claimed"], x["positives"]) == (int(pred.sum()), int((pred & same).sum()))
                        assert e["best_thres"] == _best_by_the_references_rule(ps[:, g], same, grid64)
        m._kept.drop()
