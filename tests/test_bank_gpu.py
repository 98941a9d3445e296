"""The anchor-bank audit on the GPU (memvul_amd/bank.py, include/memvul_bank.h, csrc/bank_cover.h).  The witness is the engine itself: anchor_set(V), then match(U)
gives probs[:, :, same_idx] — the bits every entry point of the engine produces for those pairs.  The marking must EQUAL (P >= t) over that matrix and the rows
ClaimIndex.select lists for the same call; totals, hist, sole, mult, sole_of, overlap and the greedy cover must equal the numpy definitions (bank_kit) over it.  The
thresholds are taken from the matrix itself (entries, and their neighbours one fp32 step up), so a single differing bit of P(same) moves a count.  There is no
tolerance in this file.

The library never hands the bit matrix out.  It is pinned two ways: every result of a marking equals the definition, and — exactly, column by column — with every
OTHER vector's threshold above 1 (it claims nothing, but keeps its place in its tile and group) ``mult`` IS the one vector's column."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import bank, claims, synth

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bank_kit as kit  # noqa: E402
import claims_kit  # noqa: E402
from kept_index_kit import L2, WK, WK768, _engine_matrix, bare_model  # noqa: E402

N_512, Q_512, N_768, Q_768 = 4099, 37, 1000, 124
ABOVE_ONE = np.nextafter(np.float32(1), np.float32(2))


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
    U, V, _ = kit.rkit.fixture(47 + P, N_512 if P == 512 else N_768, P, Q_512 if P == 512 else Q_768, block_rows=64)
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


def _entry(ps, f):
    """Per column of ps [N, Q] the order statistic at fraction f of the non-NaN column: a VALUE of the matrix, fp32 [Q]."""
    out = np.zeros(ps.shape[1], np.float32)
    for g in range(ps.shape[1]):
        col = np.sort(ps[:, g][~np.isnan(ps[:, g])])
        out[g] = col[min(len(col) - 1, int(round(f * (len(col) - 1))))] if len(col) else 0.5
    return out


def _mixed(ps):
    """One threshold per vector, all taken from the matrix: the column's 80th-percentile entry, the fp32 neighbour above its 90th-percentile entry, its 99.7th-percentile
    entry (claims_kit.matrix_thresholds column 2), in turn; the vector in the middle gets 1.0's upper neighbour and claims nothing."""
    Q = ps.shape[1]
    th = claims_kit.matrix_thresholds(ps)
    kinds = np.stack([_entry(ps, 0.8), np.nextafter(_entry(ps, 0.9), np.float32(2)), th[:, 2]], 1)
    out = kinds[np.arange(Q), np.arange(Q) % 3].astype(np.float32)
    if Q > 2:
        out[Q // 2] = th[Q // 2, 14]
    return np.ascontiguousarray(out)


class _Bite:
    """The fixture condition, gathered over the markings a test compares and asserted on the reference alone."""

    def __init__(self):
        self.nothing = self.unclaimed = self.many = self.one = False
        self.claimed = self.pairs = 0

    def see(self, B):
        m = B.sum(1)
        self.nothing = self.nothing or bool((B.sum(0) == 0).any())
        self.unclaimed = self.unclaimed or bool((m == 0).any())
        self.many = self.many or bool((m >= 2).any())
        self.one = self.one or bool((m == 1).any())
        self.claimed += int(B.sum())
        self.pairs += int(B.size)

    def check(self):
        share = self.claimed / max(self.pairs, 1)
        assert self.nothing and self.unclaimed and self.many and self.one and 0.05 < share < 0.95, (self.nothing, self.unclaimed, self.many, self.one, share)
        return share


def _index(c, same_idx, rows, set_classes=True):
    ix = bank.BankAudit(0, c["U"].shape[1], c["Wm"], same_idx)
    ix.add(np.ascontiguousarray(c["U"][:rows]))
    if set_classes:  # two overlapping calls and a third: the later ones overwrite what the first said
        want = np.array(c["cls"][:rows])
        a, b = rows * 2 // 3, rows // 3
        ix.set_classes(np.ascontiguousarray(1 - want[:a]))
        ix.set_classes(np.ascontiguousarray(want[b:]), b)
        ix.set_classes(np.ascontiguousarray(want[:b]))
    return ix


def _readers(ix):
    tot = ix.totals()
    hist, sole, mult, sole_of = ix.multiplicity(per_row=True)
    h2, s2 = ix.multiplicity()
    assert np.array_equal(h2, hist) and np.array_equal(s2, sole)
    return dict(totals=tot, hist=hist, sole=sole, mult=mult, sole_of=sole_of, overlap=ix.overlap())


KEYS = ("totals", "hist", "sole", "mult", "sole_of", "overlap")


def _compare(ix, v, thres, ps, cls, first, count, what):
    """mark + every reader against the definitions over ps[first : first + count]."""
    ix.mark(v, thres, first, count)
    got = _readers(ix)
    B = kit.marking(ps[first:first + count], thres)
    c = cls[first:first + count]
    hist, sole, mult, sole_of = kit.multiplicity(B, c)
    want = dict(totals=kit.totals(B, c), hist=hist, sole=sole, mult=mult, sole_of=sole_of, overlap=kit.overlap(B, c))
    assert kit.same(got, want, KEYS) == [], (what, first, count, kit.same(got, want, KEYS))
    Q = len(v)
    assert np.array_equal(got["overlap"][np.arange(Q), np.arange(Q)], got["totals"]) and np.array_equal(got["overlap"], got["overlap"].transpose(1, 0, 2))
    return B


def _columns(ix, v, thres, ps, first, count, which):
    """Column q of the marking, exactly: every other vector claims nothing, so mult is the column."""
    for q in which:
        alone = np.full(len(v), ABOVE_ONE, np.float32)
        alone[q] = thres[q]
        ix.mark(v, alone, first, count)
        mult = ix.multiplicity(per_row=True)[2]
        want = kit.marking(ps[first:first + count, q:q + 1], thres[q:q + 1])[:, 0]
        assert np.array_equal(mult, want.astype(np.uint16)), (q, np.flatnonzero(mult != want)[:5].tolist())


def _selection(c, same_idx, v, thres, first, count):
    """The marking that ClaimIndex.select(order="row") lists for the same call, as a boolean matrix [count, Q]."""
    with claims.ClaimIndex(0, c["U"].shape[1], c["Wm"], same_idx) as cx:
        cx.add(np.ascontiguousarray(c["U"][:first + count]))
        off, rows, _ = cx.select(v, thres, first, count, order="row")
    B = np.zeros((count, len(v)), bool)
    for q in range(len(v)):
        B[rows[off[q]:off[q + 1]] - first, q] = True
    return B


# ---- 1: the marking and its readers ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_idx", [0, 1])
def test_marking_and_readers_at_512_features(gu, c512, same_idx):
    bite = _Bite()
    with _index(c512, same_idx, N_512) as ix:
        for Q in (1, 17, Q_512):
            v = np.ascontiguousarray(c512["V"][:Q])
            ps = c512["probs"][:, :Q, same_idx]
            thres = _mixed(ps)
            for first, count in ((0, N_512), (3, 130), (0, 63), (5, 0)):
                B = _compare(ix, v, thres, ps, c512["cls"], first, count, f"Q={Q}")
                if count:
                    assert np.array_equal(B, _selection(c512, same_idx, v, thres, first, count)), (Q, first, count)  # the rows ClaimIndex.select lists
                if Q == Q_512 and count:
                    bite.see(B)
                if Q == Q_512 and count == N_512:
                    ms = {}
                    ix.mark(v, thres)
                    ms["mark"] = ix.kernel_ms()
                    ix.totals()
                    ms["totals"] = ix.kernel_ms()
                    ix.multiplicity()
                    ms["multiplicity"] = ix.kernel_ms()
                    ix.overlap()
                    ms["overlap"] = ix.kernel_ms()
                    order, _ = ix.greedy(3, 1)
                    ms["greedy"] = ix.kernel_ms() if len(order) else 0.0
                    gu.record("bank_audit", N=N_512, Q=Q, P=512, same_idx=same_idx, rounds=int(len(order)), kernel_ms=ms)
            _columns(ix, v, thres, ps, 0, N_512, range(Q) if same_idx == 0 else sorted({q for q in (0, 15, 16, Q - 1) if q < Q}))
            _columns(ix, v, thres, ps, 3, 130, (0, Q - 1))
    bite.check()


def test_marking_and_readers_at_768_features(gu, c768):
    bite = _Bite()
    v = np.ascontiguousarray(c768["V"])
    ps = c768["probs"][:, :, 0]
    thres = _mixed(ps)
    with _index(c768, 0, N_768) as ix:
        for first, count in ((0, N_768), (3, 130)):
            B = _compare(ix, v, thres, ps, c768["cls"], first, count, "P=768")
            assert np.array_equal(B, _selection(c768, 0, v, thres, first, count))
            bite.see(B)
        ix.mark(v, thres)
        ms = {"mark": ix.kernel_ms()}
        ix.multiplicity()
        ms["multiplicity"] = ix.kernel_ms()
        ix.overlap()
        ms["overlap"] = ix.kernel_ms()
        order, _ = ix.greedy(3, 1)
        ms["greedy"] = ix.kernel_ms() if len(order) else 0.0
        gu.record("bank_audit", N=N_768, Q=Q_768, P=768, same_idx=0, rounds=int(len(order)), kernel_ms=ms)
        _columns(ix, v, thres, ps, 0, N_768, (0, 15, 16, 63, 64, Q_768 - 1))
    bite.check()


# ---- 2: a NaN row, and the way the rows arrived ------------------------------------------------------------------------------------------------------------------------

def test_a_nan_row_claims_nothing(gu, c512):
    U = np.array(c512["U"][:300])
    U[200, 170] = np.float32("nan")
    V = np.ascontiguousarray(c512["V"][:7])
    probs = _engine_matrix(c512["eng"], U, V)
    assert np.isnan(probs[200]).all() and not np.isnan(np.delete(probs, 200, 0)).any()
    ps = probs[:, :, 0]
    cls = np.array(c512["cls"][:300])
    with bank.BankAudit(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        ix.set_classes(cls)
        B = _compare(ix, V, _mixed(ps), ps, cls, 0, 300, "a NaN row")
        assert not B[200].any() and B.any()
        ix.mark(V, 0.0)  # everything but the NaN row
        hist, sole, mult, sole_of = ix.multiplicity(per_row=True)
        assert mult[200] == 0 and (np.delete(mult, 200) == 7).all() and hist[:, 0].sum() == 1 and hist[:, 7].sum() == 299 and (sole == 0).all() and (sole_of == -1).all()
        assert (ix.totals().sum(1) == 299).all()


def test_rows_added_in_three_calls(gu, c512):
    N, Q = 257, 17
    v = np.ascontiguousarray(c512["V"][:Q])
    ps, cls = c512["probs"][:N, :Q, 0], c512["cls"]
    thres = _mixed(ps)
    with bank.BankAudit(0, 512, c512["Wm"], 0) as parts:
        for a, b in ((0, 1), (1, 64), (64, N)):
            parts.add(np.ascontiguousarray(c512["U"][a:b]))
        assert len(parts) == N
        parts.set_classes(np.ascontiguousarray(cls[:N]))
        for first, count in ((0, N), (1, N - 1), (63, 130), (64, 64), (N - 1, 1)):
            _compare(parts, v, thres, ps, cls, first, count, "adds of 1, 63 and the rest")
        parts.reset()
        assert len(parts) == 0
        parts.mark(v, thres)  # an empty marking: every reader returns zeros
        r = _readers(parts)
        assert all((r[k] == 0).all() for k in ("totals", "hist", "sole", "overlap")) and r["mult"].shape == (0,) and parts.greedy()[0].shape == (0,)
        parts.add(np.ascontiguousarray(c512["U"][:N]))
        parts.mark(v, thres)
        assert (parts.totals()[:, 1] == 0).all()  # the classes went with the rows
        parts.set_classes(np.ascontiguousarray(cls[:N]))
        _compare(parts, v, thres, ps, cls, 0, N, "reset then add")


# ---- 3: the plan -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_no_plan_changes_an_integer(gu, c512):
    v = np.ascontiguousarray(c512["V"])
    ps = c512["probs"][:, :, 0]
    thres = _mixed(ps)
    want_g = kit.greedy(kit.marking(ps, thres), c512["cls"], 3, 1)
    assert len(want_g[0]) >= 2
    with _index(c512, 0, N_512) as ix:
        for block_rows in (0, 64, 128, 256, 512):
            for group in (5, 16):
                for chunk in (1, 3):
                    ix.test_plan(block_rows, group, chunk)
                    _compare(ix, v, thres, ps, c512["cls"], 0, N_512, (block_rows, group, chunk))
                    order, gained = ix.greedy(3, 1)
                    assert np.array_equal(order, want_g[0]) and np.array_equal(gained, want_g[1]), (block_rows, group, chunk)
                    _compare(ix, v, thres, ps, c512["cls"], 3, 130, (block_rows, group, chunk))
        ix.test_plan(64, 16, 2)
        _columns(ix, v, thres, ps, 0, N_512, (0, 4, 5, 15, 16, 31, 32, Q_512 - 1))


# ---- 4: the greedy cover -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Q", [(N_512, Q_512), (1000, 19)])
def test_the_greedy_cover(gu, c512, N, Q):
    v = np.ascontiguousarray(c512["V"][:Q])
    ps = c512["probs"][:N, :Q, 0]
    thres = np.ascontiguousarray(_entry(ps, 0.9))
    B = kit.marking(ps, thres)
    cls = ((B.sum(1) >= 1) ^ (np.random.default_rng(5).random(N) < 0.15)).astype(np.uint8)
    assert np.array_equal(v[3], v[1]) and (Q != Q_512 or np.array_equal(v[Q - 1], v[0]))  # the fixture's duplicate vectors: exact ties
    ref = kit.greedy(B, cls, 1, 1)
    assert len(ref[0]) >= 8 and ref[2] >= 1, (len(ref[0]), ref[2])  # on the reference alone: enough rounds, and a tied one
    fixed = np.zeros(Q, np.uint8)
    fixed[[int(ref[0][0]), int(ref[0][2]), Q - 1]] = 1
    with bank.BankAudit(0, 512, c512["Wm"], 0) as ix:
        ix.add(np.ascontiguousarray(c512["U"][:N]))
        ix.set_classes(cls)
        ix.mark(v, thres)
        assert np.array_equal(ix.totals(), kit.totals(B, cls))
        for kw in (dict(w_pos=1, w_neg=1), dict(w_pos=3, w_neg=1), dict(w_pos=1, w_neg=1, fixed=fixed), dict(w_pos=1, w_neg=1, max_rounds=3), dict(w_pos=0, w_neg=1),
                   dict(w_pos=2 ** 20, w_neg=2 ** 20), dict(w_pos=1, w_neg=0)):
            want = kit.greedy(B, cls, kw["w_pos"], kw["w_neg"], kw.get("fixed"), kw.get("max_rounds"))
            order, gained = ix.greedy(**kw)
            assert order.dtype == np.int32 and gained.dtype == np.int64 and np.array_equal(order, want[0]) and np.array_equal(gained, want[1]), (kw, order.tolist(), want[0].tolist())
            if kw == dict(w_pos=1, w_neg=1):
                gu.record("bank_greedy", N=N, Q=Q, P=512, rounds=int(len(order)), tied_rounds=int(want[2]), kernel_ms=ix.kernel_ms())
            if "fixed" in kw:
                assert not set(order.tolist()) & set(np.flatnonzero(fixed).tolist()) and len(order) >= 1
            if "max_rounds" in kw:
                assert len(order) == 3
            if kw["w_pos"] == 0:
                assert len(order) == 0
        assert np.array_equal(ix.totals(), kit.totals(B, cls))  # the readers left the marking alone


# ---- 5: the held marking and the refusals ------------------------------------------------------------------------------------------------------------------------------

def test_the_held_marking_and_the_refusals(gu, c512):
    """The rule of include/memvul_bank.h: the readers follow a successful mvb_mark as often as asked; mvb_count, mvb_kernel_ms and mvb_last_error leave the marking
    alone; every other call on the index drops it.  A refused call leaves its outputs untouched."""
    N, Q = 257, 7
    v = np.zeros((4097, 512), np.float32)
    v[:Q] = c512["V"][:Q]
    ps = c512["probs"][:N, :Q, 0]
    thres = _mixed(ps)
    th = np.full(4097, 0.5, np.float32)
    th[:Q] = thres
    with _index(c512, 0, N) as ix:
        lib, h = ix._lib, ix._h
        out = np.full(4097 * 2, 7, np.int64)
        big = np.full(Q * Q * 2, 7, np.int64)
        rounds, order, gained = C.c_int(7), np.full(Q, 7, np.int32), np.full(2 * Q, 7, np.int64)
        vp, tp, op, bp = (a.ctypes.data_as(C.c_void_p) for a in (v, th, out, big))

        def untouched():
            return (out == 7).all() and (big == 7).all() and rounds.value == 7 and (order == 7).all() and (gained == 7).all()

        def no_marking():
            for rc in (lib.mvb_totals(h, op), lib.mvb_multiplicity(h, op, op, None, None), lib.mvb_overlap(h, bp),
                       lib.mvb_greedy(h, 1, 1, None, Q, C.byref(rounds), order.ctypes.data_as(C.c_void_p), gained.ctypes.data_as(C.c_void_p))):
                assert rc == bank.ERR_STATE and b"no marking is held" in lib.mvb_last_error(h) and untouched()

        def refused(rc, words):
            msg = lib.mvb_last_error(h)
            assert rc == -1 and words in msg and untouched(), (rc, msg)

        no_marking()  # nothing marked yet
        B = _compare(ix, np.ascontiguousarray(v[:Q]), thres, ps, c512["cls"], 0, N, "held")
        assert len(ix) == N and ix.kernel_ms() > 0
        want_t = kit.totals(B, c512["cls"][:N])
        for _ in range(2):  # as often as asked, in any order, and after the calls that leave it alone
            assert np.array_equal(ix.overlap()[np.arange(Q), np.arange(Q)], want_t) and np.array_equal(ix.totals(), want_t) and len(ix) == N
        # refusals of a reader leave the marking where it is
        refused(lib.mvb_greedy(h, 2 ** 20 + 1, 1, None, Q, C.byref(rounds), order.ctypes.data_as(C.c_void_p), gained.ctypes.data_as(C.c_void_p)), b"w_pos = 1048577")
        refused(lib.mvb_greedy(h, 1, -1, None, Q, C.byref(rounds), order.ctypes.data_as(C.c_void_p), gained.ctypes.data_as(C.c_void_p)), b"w_neg = -1")
        refused(lib.mvb_greedy(h, 1, 1, None, -1, C.byref(rounds), order.ctypes.data_as(C.c_void_p), gained.ctypes.data_as(C.c_void_p)), b"max_rounds = -1")
        refused(lib.mvb_greedy(h, 1, 1, None, Q, None, order.ctypes.data_as(C.c_void_p), gained.ctypes.data_as(C.c_void_p)), b"NULL")
        refused(lib.mvb_totals(h, None), b"NULL")
        refused(lib.mvb_multiplicity(h, None, op, None, None), b"NULL")
        refused(lib.mvb_overlap(h, None), b"NULL")
        refused(lib.mvb_kernel_ms(h, None), b"NULL")
        assert np.array_equal(ix.totals(), want_t)
        # every other call drops it, whether or not it succeeds
        drops = (lambda: ix.reset(), lambda: ix.add(np.ascontiguousarray(c512["U"][:N])), lambda: ix.set_classes(np.zeros(3, np.uint8)), lambda: ix.test_plan(0, 0, 0),
                 lambda: lib.mvb_mark(h, vp, 0, tp, 0, N), lambda: lib.mvb_set_classes(h, None, 0, 3), lambda: lib.mvb_test_plan(h, 100, 0, 0))
        for drop in drops:
            if len(ix):
                ix.mark(np.ascontiguousarray(v[:Q]), thres)
            drop()
            no_marking()
        # refused markings
        nan_th, inf_th = th.copy(), th.copy()
        nan_th[2], inf_th[0] = np.float32("nan"), np.float32("inf")
        refused(lib.mvb_mark(h, vp, 0, tp, 0, N), b"Q = 0")
        refused(lib.mvb_mark(h, vp, 4097, tp, 0, N), b"Q = 4097")
        refused(lib.mvb_mark(h, vp, 3, nan_th.ctypes.data_as(C.c_void_p), 0, N), b"thres[2] is not finite")
        refused(lib.mvb_mark(h, vp, 3, inf_th.ctypes.data_as(C.c_void_p), 0, N), b"thres[0] is not finite")
        refused(lib.mvb_mark(h, vp, 3, tp, 2, N - 1), b"rows [")
        refused(lib.mvb_mark(h, vp, 3, tp, -1, 5), b"rows [")
        refused(lib.mvb_mark(h, None, 3, tp, 0, N), b"NULL")
        refused(lib.mvb_mark(h, vp, 3, None, 0, N), b"NULL")
        refused(lib.mvb_add(h, vp, 2 ** 31), b"2^31 - 2")
        refused(lib.mvb_add(h, vp, -1), b"n = -1")
        for plan in ((100, 0, 0), (64, -1, 0), (64, 4097, 0), (64, 0, -1)):
            refused(lib.mvb_test_plan(h, *plan), b"= ")
        assert lib.mvb_mark(None, vp, 3, tp, 0, N) != 0 and b"index is NULL" in lib.mvb_last_error(None)
        no_marking()
        # an empty range holds an empty marking, and the index still answers
        ix.mark(np.ascontiguousarray(v[:Q]), thres, N, 0)
        assert (ix.totals() == 0).all() and (ix.overlap() == 0).all() and ix.greedy()[0].shape == (0,)
        ix.set_classes(np.ascontiguousarray(c512["cls"][:N]))  # (they went with the rows at the reset above)
        _compare(ix, np.ascontiguousarray(v[:Q]), thres, ps, c512["cls"], 0, N, "after the refusals")
    lib = bank.load_library()
    hh = C.c_void_p()
    for args, words in (((0, 500, 0), b"512"), ((0, 512, 2), b"same_idx"), ((4096, 512, 0), b"device")):
        assert lib.mvb_create(args[0], args[1], c512["Wm"].ctypes.data_as(C.c_void_p), args[2], C.byref(hh)) != 0 and not hh.value
        assert words in lib.mvb_last_error(None), lib.mvb_last_error(None)
    assert lib.mvb_create(0, 512, None, 0, C.byref(hh)) != 0 and b"NULL" in lib.mvb_last_error(None)


# ---- 6: end to end -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_from_a_kept_sweep(gu, c512):
    eng = c512["eng"]
    dims, _ = gu.weights_for(L2, WK)
    n = 200
    ids, lens = synth.make_ids(n, 64, dims.vocab_size, seed=synth.SEED + 77, ragged=True, min_len=3)
    same = np.random.default_rng(9).random(n) < 0.3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng.anchor_reset()
        eng.anchor_append(*synth.make_ids(5, 64, dims.vocab_size, seed=synth.SEED + 78, ragged=True, min_len=16))
        m = bare_model(eng, c512["Wm"], 5)
        arrays = {"type": "test", "ids": ids, "lens": lens, "same": same, "urls": [f"https://example.invalid/issues/{i}" for i in range(n)]}
        m.sweep_arrays(arrays, batch_size=64, with_probs=True, keep=True)
        ps = m.rematch_arrays(arrays, with_probs=True)[2]
        thres = [float(x) for x in _entry(ps, 0.8)]
        B = ps.astype(np.float64) >= np.asarray(thres)[None, :]  # the reference's comparison
        pred = B.any(1)
        assert 0.05 < B.mean() < 0.95 and pred.any() and not pred.all()
        doc = m.anchor_bank_audit(arrays, thres, w_pos=2, w_neg=1)
        assert (doc["union"]["TP"], doc["union"]["FP"], doc["union"]["FN"], doc["union"]["TN"]) == (
            int((pred & same).sum()), int((pred & ~same).sum()), int((~pred & same).sum()), int((~pred & ~same).sum()))
        for g, a in enumerate(doc["anchors"]):
            only = B[:, g] & (B.sum(1) == 1)
            assert a["anchor"] == f"CWE-{g}" and a["claimed"] == [int((B[:, g] & ~same).sum()), int((B[:, g] & same).sum())]
            assert a["sole"] == [int((only & ~same).sum()), int((only & same).sum())]
        order, gained, _ = kit.greedy(B, same.astype(np.uint8), 2, 1)
        assert [x["index"] for x in doc["greedy"]] == order.tolist() and [[x["new_pos"], x["new_neg"]] for x in doc["greedy"]] == gained.tolist()
        index = m._kept.indexes["bank"]
        cand = np.ascontiguousarray(eng.anchor_get()[[1, 0, 2]] * np.float32(0.75))  # (stand-ins for the embeddings of fresh descriptions)
        doc2 = m.anchor_bank_audit(arrays, thres, candidates=cand, candidate_thres=thres[0], w_pos=2, w_neg=1)
        assert m._kept.indexes["bank"] is index and doc2["union"] == doc["union"] and len(doc2["candidates"]) == 3
        assert all(0 <= x["index"] < 3 and x["anchor"] == f"candidate {x['index']}" for x in doc2["greedy"])
        m._kept.drop()
        assert m._kept.indexes["bank"] is None
