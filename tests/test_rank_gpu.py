"""Per-anchor ranking quality on the GPU (memvul_amd/rank.py, include/memvul_rank.h, csrc/rank_sort.h).  The witness is the engine itself: anchor_set(V), then
match(U) gives probs[:, :, same_idx] — the bits every entry point of the engine produces for those pairs.  The integers (n, u2, best, the curve's tp / fp) and the
fp32 values (best_thres, the curve's thres) must be BYTE-EQUAL to rank_kit.reference_rank / reference_curve on that matrix: no tolerance.  ap must be bit-equal across
every plan and within (D + 3) 2^-53 of the exact fraction (D non-negative terms of at most three roundings each and D - 1 additions, the sum at most 1).

Every test first asserts, on the reference alone, that its rankings bite: some compared ranking has a tie group holding both classes, some has its best cut strictly
inside, and the compared AUCs lie on both sides of 0.5."""
import ctypes as C
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

from memvul_amd import claims, rank, synth

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_kit as kit  # noqa: E402
from kept_index_kit import L2, WK, WK768, _engine_matrix, _same_bytes, bare_model  # noqa: E402

N_PLAN, N_MAX, Q_MAX, Q_768, Q_PLAN = 4099, 1000, 33, 124, 7
KINDS = ("zeros", "ones", "alternating", "random", "informative")


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


def _case(gu, P):
    """Once per embedding width: the fixture of the claims tests, the engine's matcher weight, and the engine's own probabilities of all pairs (shared, read-only)."""
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
    return dict(eng=eng, Wm=Wm, U=U, V=V, probs=probs, cls=cls, refs={})


@pytest.fixture(scope="module")
def c512(gu):
    return _case(gu, 512)


@pytest.fixture(scope="module")
def c768(gu):
    return _case(gu, 768)


def _classes(kind, c, N, same_idx):
    """The first N of the case's classes under an assignment (each is defined over ALL rows of the case, so that every prefix and range sees the same classes)."""
    rows = len(c["probs"])
    flip = np.random.default_rng(17).random(rows) < 0.1
    p0 = c["probs"][:, 0, same_idx]
    if kind == "zeros":
        cls = np.zeros(rows, np.uint8)
    elif kind == "ones":
        cls = np.ones(rows, np.uint8)
    elif kind == "alternating":
        cls = (np.arange(rows) % 2).astype(np.uint8)
    elif kind == "random":
        cls = np.array(c["cls"])
    elif kind == "informative":  # the score of vector 0 above its median, 10 % flipped — the best cut is interior
        cls = ((p0 > np.median(p0)) ^ flip).astype(np.uint8)
    else:
        # contrast: vector 0 scores the row above vector 5 (above its own median, where there are fewer vectors), 10 % flipped — vector 0 ranks the positives up,
        # vector 5 ranks them down; and the fixture's duplicate rows (2, 3) and (63, 64) in opposite classes: tie groups that hold both
        other = c["probs"][:, 5, same_idx] if c["probs"].shape[1] > 5 else np.median(p0)
        cls = ((p0 > other) ^ flip).astype(np.uint8)
        for a, b in ((2, 3), (63, 64)):
            cls[a], cls[b] = 0, 1
    return np.ascontiguousarray(cls[:N])


def _index(c, same_idx, rows, cls=None):
    ix = rank.RankIndex(0, c["U"].shape[1], c["Wm"], same_idx)
    ix.add(np.ascontiguousarray(c["U"][:rows]))
    if cls is not None:
        ix.set_classes(np.ascontiguousarray(cls[:rows]))
    return ix


class _Bite:
    """The fixture conditions, gathered over the rankings a test compares and asserted on the reference alone."""

    def __init__(self):
        self.mixed = self.interior = self.above = self.below = 0

    def see(self, exact):
        for e in exact:
            self.mixed += e["mixed"] > 0
            self.interior += bool(e["interior"])
            auc = rank.auc_of(e["u2"], e["n"][1], e["n"][0])
            if auc is not None:
                self.above += auc > 0.5
                self.below += auc < 0.5

    def check(self):
        assert self.mixed and self.interior and self.above and self.below, (self.mixed, self.interior, self.above, self.below)


def _reference(c, same_idx, first, count, Q, kind, bank=True):
    """reference_matrix of rows [first, first + count) against the first Q vectors; every column's ranking is computed once per case and shared."""
    ps = c["probs"][:, :, same_idx]
    cls = _classes(kind, c, len(ps), same_idx)[first:first + count]
    keys = [("col", same_idx, first, count, q, kind) for q in range(Q)] + ([("bank", same_idx, first, count, Q, kind)] if bank else [])
    for key in keys:
        if key not in c["refs"]:
            col = ps[first:first + count, key[4]] if key[0] == "col" else kit.bank_scores(ps[first:first + count, :Q])
            c["refs"][key] = kit.reference_rank(col, cls)
    exact = [c["refs"][key] for key in keys]
    return dict(n=np.array([e["n"] for e in exact], np.int64).reshape(-1, 3), u2=np.array([e["u2"] for e in exact], np.int64),
                best_thres=np.array([e["best_thres"] for e in exact], np.float32), best=np.array([e["best"] for e in exact], np.int64).reshape(-1, 2), exact=exact)


def _witnesses(c, same_idx, ranges, Q, kinds=("informative", "contrast"), bank=True):
    """{(kind, first, count): _reference}, after the fixture conditions were asserted over all of them."""
    bite, out = _Bite(), {}
    for kind in kinds:
        for first, count in ranges:
            out[kind, first, count] = _reference(c, same_idx, first, count, Q, kind, bank)
            bite.see(out[kind, first, count]["exact"])
    bite.check()
    return out


def _compare(got, want, what):
    """Integers and fp32 values byte-equal; ap within its bound of the exact fraction, NaN exactly where there is no positive; auc by Python-int division."""
    for k in ("n", "u2", "best"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k)
        if not np.array_equal(got[k], want[k]):
            at = np.argwhere(got[k] != want[k])[:4].tolist()
            print(f"{what}: {k} differs at {at}: got {[got[k][tuple(i)].item() for i in at]}, want {[want[k][tuple(i)].item() for i in at]}")
        assert np.array_equal(got[k], want[k]), (what, k)
    _same_bytes(got["best_thres"], want["best_thres"], f"{what}: best_thres")
    assert got["ap"].dtype == np.float64 and got["ap"].shape == want["u2"].shape
    worst = Fraction(0)
    for s, e in enumerate(want["exact"]):
        if e["ap"] is None:
            assert np.isnan(got["ap"][s]) and got["auc"][s] is None, (what, s)
            continue
        err = abs(Fraction(float(got["ap"][s])) - e["ap"])
        worst = max(worst, err / kit.ap_bound(e))
        assert err <= kit.ap_bound(e), (what, s, float(got["ap"][s]), float(e["ap"]), float(err), float(kit.ap_bound(e)))
        assert got["auc"][s] == rank.auc_of(e["u2"], e["n"][1], e["n"][0])
    return float(worst)


# ---- 1: every size, every class assignment ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_idx", [0, 1])
def test_rank_is_the_matrix_ranked(gu, c512, same_idx):
    sizes = {N: ((33,) if N == 4099 else (1, 15, 16, 17, 33)) for N in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099)}
    kinds = {1000: ("ones", "random", "informative"), 4099: ("alternating", "informative")}  # (every assignment at the small sizes; the references are exact fractions)
    cases, bite = [], _Bite()
    for N, Qs in sizes.items():
        for kind in kinds.get(N, KINDS):
            for Q in Qs:
                want = _reference(c512, same_idx, 0, N, Q, kind)
                bite.see(want["exact"])
                cases.append((N, kind, Q, want))
    bite.check()
    worst = 0.0
    for N in sizes:
        with _index(c512, same_idx, N) as ix:
            last = None
            for n, kind, Q, want in cases:
                if n != N:
                    continue
                if kind != last:
                    if kind != "zeros":  # (a fresh index's classes are 0)
                        ix.set_classes(_classes(kind, c512, N, same_idx))
                    last = kind
                got = ix.rank(np.ascontiguousarray(c512["V"][:Q]), bank=True)
                if Q == 33 and kind == "random":  # (one figure per size: the records are read by people)
                    gu.record("rank_rank", N=N, Q=Q, P=512, same_idx=same_idx, **ix.stage_ms())
                worst = max(worst, _compare(got, want, f"N={N} Q={Q} {kind}"))
    gu.record("rank_ap_error", same_idx=same_idx, worst_share_of_bound=worst)


@pytest.mark.parametrize("N,Q", [(65, 3), (1000, 124)])
def test_rank_and_curve_at_768_features(gu, c768, N, Q):
    bite = _Bite()
    for same_idx in (0, 1):
        for kind in ("random", "contrast"):
            bite.see(_reference(c768, same_idx, 0, N, Q, kind)["exact"])
    bite.check()
    v = np.ascontiguousarray(c768["V"][:Q])
    for same_idx in (0, 1):
        with _index(c768, same_idx, N) as ix:
            for kind in ("random", "contrast"):
                cls = _classes(kind, c768, N, same_idx)
                ix.set_classes(cls)
                got = ix.rank(v, bank=True)
                gu.record("rank_rank", N=N, Q=Q, P=768, same_idx=same_idx, classes=kind, **ix.stage_ms())
                _compare(got, _reference(c768, same_idx, 0, N, Q, kind), f"P=768 N={N} Q={Q} {kind}")
            ps = c768["probs"][:N, :Q, same_idx]
            for col, curve in ((ps[:, 1], ix.curve(np.ascontiguousarray(v[1:2]))), (kit.bank_scores(ps), ix.curve(v, bank=True))):
                want = kit.reference_curve(col, cls)
                _same_bytes(curve[0], want[0], "curve thres")
                assert np.array_equal(curve[1], want[1]) and np.array_equal(curve[2], want[2]) and curve[1].dtype == curve[2].dtype == np.int64


# ---- 2: the plan, sub-ranges, the way the rows arrived ------------------------------------------------------------------------------------------------------------------

RANGES = ((0, N_PLAN), (63, 130), (1, N_PLAN - 1), (1000, 300), (65, 64), (N_PLAN - 1, 1), (5, 0))


def test_no_plan_changes_a_byte(gu, c512):
    Q = Q_MAX
    v = np.ascontiguousarray(c512["V"][:Q])
    wants, bite = {}, _Bite()
    for first, count in RANGES:
        wants[first, count] = _reference(c512, 0, first, count, Q, "contrast")
        bite.see(wants[first, count]["exact"])
    bite.check()
    with _index(c512, 0, N_PLAN, _classes("contrast", c512, N_PLAN, 0)) as ix:
        aps = {}
        for tile in (256, 1024, 0, 512):
            for group in (1, 16, 17, 0):
                ix.test_plan(tile, group)
                for (first, count), want in wants.items():
                    if (first, count) != (0, N_PLAN) and (group == 1 or tile == 512):  # (the sub-ranges under three of the four groupings)
                        continue
                    got = ix.rank(v, first, count, bank=True)
                    if (first, count) == (0, N_PLAN):
                        gu.record("rank_plan", plan=[tile, group], **ix.stage_ms())
                    _compare(got, want, f"plan ({tile}, {group}) rows [{first}, +{count})")
                    ap = aps.setdefault((first, count), got["ap"])
                    assert got["ap"].tobytes() == ap.tobytes(), (tile, group, first, count)  # bit-equal across every plan
                for q, bank in ((5, False), (0, True)):
                    curve = ix.curve(v if bank else np.ascontiguousarray(v[q:q + 1]), bank, 63, 1300)
                    ps = c512["probs"][63:1363, :Q, 0]
                    want = kit.reference_curve(kit.bank_scores(ps) if bank else ps[:, q], _classes("contrast", c512, N_PLAN, 0)[63:1363])
                    _same_bytes(curve[0], want[0], f"plan ({tile}, {group}) curve thres")
                    assert np.array_equal(curve[1], want[1]) and np.array_equal(curve[2], want[2]), (tile, group, bank)
        # a cap that holds three vectors at a time, then the refusal below one vector's need: the figure in the message, nothing allocated, the outputs untouched
        ix.test_plan(256, 0, 3 * 60000 + 4 * N_PLAN)
        _compare(ix.rank(v, bank=True), wants[0, N_PLAN], "a cap of three vectors")
        ix.test_plan(0, 0, 20000)
        lib, h = ix._lib, ix._h
        out = [np.full(3 * (Q + 1), 7, np.int64), np.full(Q + 1, 7, np.int64), np.full(Q + 1, 7.0, np.float64), np.full(Q + 1, 7.0, np.float32), np.full(2 * (Q + 1), 7, np.int64)]
        rc = lib.mvk_rank(h, v.ctypes.data_as(C.c_void_p), Q, 1, 0, N_PLAN, *(a.ctypes.data_as(C.c_void_p) for a in out))
        msg = lib.mvk_last_error(h)
        assert rc == -1 and b"the cap is 20000" in msg and str(N_PLAN).encode() in msg and all((a == 7).all() for a in out), (rc, msg)
        assert lib.mvk_curve(h, v.ctypes.data_as(C.c_void_p), Q, 1, 0, N_PLAN, C.byref(C.c_int64())) == -1 and b"the cap is 20000" in lib.mvk_last_error(h)
        _compare(ix.rank(v, 65, 64, bank=True), wants[65, 64], "a range that fits the small cap")  # and the index still answers
        with pytest.raises(RuntimeError, match="the cap is"):
            ix.rank(v)


def test_the_way_the_rows_arrived(gu, c512):
    N, Q = 257, Q_PLAN
    v = np.ascontiguousarray(c512["V"][:Q])
    cls = _classes("contrast", c512, N_PLAN, 0)
    ranges = ((0, N), (1, N - 1), (63, 130), (64, 64), (N - 1, 1), (5, 0))
    both = _witnesses(c512, 0, ranges, Q)
    wants = {r: both["contrast", r[0], r[1]] for r in ranges}
    with rank.RankIndex(0, 512, c512["Wm"], 0) as parts:
        for a, b in ((0, 1), (1, 64), (64, N)):
            parts.add(np.ascontiguousarray(c512["U"][a:b]))
        assert len(parts) == N
        parts.set_classes(np.ascontiguousarray(1 - cls[:200]))  # two overlapping calls: the second overwrites the tail of the first
        parts.set_classes(np.ascontiguousarray(cls[100:N]), 100)
        parts.set_classes(np.ascontiguousarray(cls[:100]))
        for (first, count), want in wants.items():
            _compare(parts.rank(v, first, count, bank=True), want, f"adds of 1, 63 and the rest: rows [{first}, +{count})")
        parts.reset()
        assert len(parts) == 0
        empty = parts.rank(v, bank=True)
        assert (empty["n"] == 0).all() and (empty["u2"] == 0).all() and np.isnan(empty["ap"]).all() and np.isnan(empty["best_thres"]).all() and (empty["best"] == 0).all()
        assert empty["auc"] == [None] * (Q + 1) and [len(a) for a in parts.curve(v, bank=True)] == [0, 0, 0]
        parts.add(np.ascontiguousarray(c512["U"][:N]))
        assert (parts.rank(v)["n"][:, 1] == 0).all()  # the classes went with the rows
        parts.set_classes(_classes("informative", c512, N, 0))
        for first, count in ranges:
            _compare(parts.rank(v, first, count, bank=True), both["informative", first, count], f"reset then add: rows [{first}, +{count})")
        parts.set_classes(np.ascontiguousarray(cls[:N]))
        _compare(parts.rank(v, bank=True), wants[0, N], "the first classes again")
        # the vectors do not see each other: a vector alone, first, last, and twice
        whole = parts.rank(v)
        for q in (0, 3, Q - 1):
            for vv, at in ((v[q:q + 1], 0), (np.concatenate([v[:5], v[q:q + 1]]), 5), (np.concatenate([v[q:q + 1], v[q:q + 1]]), 1)):
                one = parts.rank(np.ascontiguousarray(vv))
                for k in ("n", "u2", "ap", "best_thres", "best"):
                    assert one[k][at].tobytes() == whole[k][q].tobytes(), (q, at, k)


# ---- 3: special rows ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_nan_row_is_left_out_and_counted(gu, c512):
    U = np.array(c512["U"][:300])
    U[200, 170] = np.float32("nan")
    V = np.ascontiguousarray(c512["V"][:Q_PLAN])
    probs = _engine_matrix(c512["eng"], U, V)
    assert np.isnan(probs[200]).all() and not np.isnan(np.delete(probs, 200, 0)).any()
    ps = np.ascontiguousarray(probs[:, :, 0])
    cols = [ps[:, q] for q in range(Q_PLAN)] + [kit.bank_scores(ps)]
    bite, wants = _Bite(), {}
    for kind in ("informative", "contrast"):
        cls = _classes(kind, c512, 300, 0)
        cls[200] = 1
        exact = [kit.reference_rank(col, cls) for col in cols]
        bite.see(exact)
        wants[kind] = (cls, dict(n=np.array([e["n"] for e in exact], np.int64), u2=np.array([e["u2"] for e in exact], np.int64),
                                 best_thres=np.array([e["best_thres"] for e in exact], np.float32), best=np.array([e["best"] for e in exact], np.int64), exact=exact))
        assert (wants[kind][1]["n"][:, 2] == 1).all() and (wants[kind][1]["n"].sum(1) == 300).all()
    bite.check()
    with rank.RankIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        for kind, (cls, want) in wants.items():
            ix.set_classes(cls)
            for tile in (256, 0):
                ix.test_plan(tile, 0)
                _compare(ix.rank(V, bank=True), want, f"a NaN row, {kind}, tile {tile}")
                thres, tp, fp = ix.curve(V, bank=True)
                w = kit.reference_curve(cols[-1], cls)
                _same_bytes(thres, w[0], "curve with a NaN row")
                assert np.array_equal(tp, w[1]) and np.array_equal(fp, w[2]) and tp[-1] + fp[-1] == 299 and not np.isnan(thres).any()


def test_one_tie_group_over_every_tile(gu, c512):
    """Every row a copy of one row: one tie group over all 17 tiles of 256 rows — u2 = n_pos n_neg, ap = n_pos / n, one curve point.  Beside it the fixture's own
    rows, whose rankings carry the fixture conditions."""
    N = N_PLAN
    U = np.ascontiguousarray(np.repeat(c512["U"][7:8], N, 0))
    V = np.ascontiguousarray(c512["V"][:Q_PLAN])
    one = _engine_matrix(c512["eng"], np.ascontiguousarray(U[:1]), V)[0, :, 0]
    cls = np.array(c512["cls"][:N])
    n_pos, n_neg = int(cls.sum()), int(N - cls.sum())
    beside = _witnesses(c512, 0, ((0, 257),), Q_PLAN)
    e = kit.reference_rank(np.full(N, one[0], np.float32), cls)
    assert e["groups"] == 1 and e["mixed"] == 1 and e["u2"] == n_pos * n_neg and e["ap"] == Fraction(n_pos, N) and e["best"] == (n_pos, n_neg)
    with rank.RankIndex(0, 512, c512["Wm"], 0) as ix:
        ix.add(U)
        ix.set_classes(cls)
        for tile in (256, 1024):
            ix.test_plan(tile, 0)
            got = ix.rank(V, bank=True)
            assert (got["n"] == [n_neg, n_pos, 0]).all() and (got["u2"] == n_pos * n_neg).all() and (got["best"] == [n_pos, n_neg]).all() and got["auc"] == [0.5] * (Q_PLAN + 1)
            _same_bytes(got["best_thres"], np.ascontiguousarray(np.concatenate([one, [one.max()]]).astype(np.float32)), "one tie group: best_thres")
            assert all(abs(Fraction(float(a)) - Fraction(n_pos, N)) <= Fraction(4, 2 ** 53) for a in got["ap"]), got["ap"]
            for q in range(2):
                thres, tp, fp = ix.curve(np.ascontiguousarray(V[q:q + 1]))
                assert thres.tobytes() == one[q:q + 1].tobytes() and tp.tolist() == [n_pos] and fp.tolist() == [n_neg]
        with _index(c512, 0, 257) as ix2:
            for (kind, _, _), want in beside.items():
                ix2.set_classes(_classes(kind, c512, 257, 0))
                _compare(ix2.rank(V, bank=True), want, f"the fixture's rows beside it, {kind}")


# ---- 4: the held curve, the other library, strictness -----------------------------------------------------------------------------------------------------------------------

def test_the_held_curve(gu, c512):
    """The rule of include/memvul_rank.h: mvk_fetch follows a successful mvk_curve as often as asked; mvk_count, mvk_kernel_ms and mvk_last_error leave the curve
    alone; every other call on the index drops it."""
    N = 257
    v = np.ascontiguousarray(c512["V"][:Q_PLAN])
    cls = _classes("contrast", c512, N, 0)
    ranked = _witnesses(c512, 0, ((0, N),), Q_PLAN)
    want = kit.reference_curve(c512["probs"][:N, 2, 0], cls)
    D = len(want[0])
    with _index(c512, 0, N) as ix:
        for (kind, _, _), w in ranked.items():  # (contrast last: its classes stay)
            ix.set_classes(_classes(kind, c512, N, 0))
            _compare(ix.rank(v, bank=True), w, f"the rankings the curve is one of, {kind}")
        lib, h = ix._lib, ix._h
        bufs = [np.full(N, 7.0, np.float32), np.full(N, 7, np.int64), np.full(N, 7, np.int64)]

        def no_curve():
            rc = lib.mvk_fetch(h, *(b.ctypes.data_as(C.c_void_p) for b in bufs))
            assert rc == rank.ERR_STATE and b"no curve is held" in lib.mvk_last_error(h) and all((b == 7).all() for b in bufs)
            with pytest.raises(RuntimeError, match="no curve is held"):
                ix.fetch()

        no_curve()  # nothing held yet
        thres, tp, fp = ix.curve(np.ascontiguousarray(v[2:3]))
        assert len(ix) == N and ix.kernel_ms() > 0 and len(thres) == D
        for _ in range(2):  # as often as asked, and after the calls that leave it alone
            t2, a2, b2 = ix.fetch()
            assert t2.tobytes() == want[0].tobytes() and np.array_equal(a2, want[1]) and np.array_equal(b2, want[2])
        ix.rank(v)
        no_curve()  # a rank call in between
        for drop in (lambda: ix.reset(), lambda: ix.add(np.ascontiguousarray(c512["U"][:N])), lambda: ix.set_classes(np.zeros(3, np.uint8)), lambda: ix.test_plan(0, 0)):
            if len(ix):
                ix.curve(np.ascontiguousarray(v[2:3]))
            drop()
            no_curve()
        assert [len(a) for a in ix.curve(v, True, N, 0)] == [0, 0, 0] and lib.mvk_fetch(h, None, None, None) == 0  # an empty range: an empty curve is held
        assert lib.mvk_curve(h, v.ctypes.data_as(C.c_void_p), 2, 0, 0, N, C.byref(C.c_int64())) != 0 and b"ONE ranking" in lib.mvk_last_error(h)
        no_curve()  # a refused curve holds nothing either


def test_the_best_cut_is_what_the_claims_library_counts(gu, c512):
    N, Q = N_MAX, Q_MAX
    v = np.ascontiguousarray(c512["V"][:Q])
    cls = _classes("contrast", c512, N, 0)
    want = _witnesses(c512, 0, ((0, N),), Q, kinds=("contrast",), bank=False)["contrast", 0, N]
    with _index(c512, 0, N, cls) as ix, claims.ClaimIndex(0, 512, c512["Wm"], 0) as cx:
        cx.add(np.ascontiguousarray(c512["U"][:N]))
        cx.set_classes(cls)
        got = ix.rank(v)
        _compare(got, want, "the ranking")
        for q0 in range(0, Q, 11):
            counts = cx.counts(np.ascontiguousarray(v[q0:q0 + 11]), np.ascontiguousarray(got["best_thres"][q0:q0 + 11]))
            for j in range(counts.shape[0]):
                assert counts[j, j].tolist() == [int(got["best"][q0 + j, 1]), int(got["best"][q0 + j, 0])], (q0, j)  # (FP, TP)


def test_strictness(gu, c512):
    lib = rank.load_library()
    h = C.c_void_p()
    for args, words in (((0, 500, 0), b"512"), ((0, 512, 2), b"same_idx"), ((4096, 512, 0), b"device")):
        assert lib.mvk_create(args[0], args[1], c512["Wm"].ctypes.data_as(C.c_void_p), args[2], C.byref(h)) != 0 and not h.value
        assert words in lib.mvk_last_error(None), lib.mvk_last_error(None)
    assert lib.mvk_create(0, 512, None, 0, C.byref(h)) != 0 and b"NULL" in lib.mvk_last_error(None)
    N, Q = 300, Q_PLAN
    cls = _classes("contrast", c512, N, 0)
    ranked = _witnesses(c512, 0, ((0, N),), Q)
    want = ranked["contrast", 0, N]
    with _index(c512, 0, N, _classes("informative", c512, N, 0)) as ix:
        _compare(ix.rank(np.ascontiguousarray(c512["V"][:Q]), bank=True), ranked["informative", 0, N], "before the refusals")
        ix.set_classes(cls)
        hh = ix._h
        v = np.zeros((4097, 512), np.float32)
        v[:Q] = c512["V"][:Q]
        out = [np.full(3 * 4098, 7, np.int64), np.full(4098, 7, np.int64), np.full(4098, 7.0, np.float64), np.full(4098, 7.0, np.float32), np.full(2 * 4098, 7, np.int64)]
        vp = v.ctypes.data_as(C.c_void_p)
        op = [a.ctypes.data_as(C.c_void_p) for a in out]
        cls2 = np.array([0, 1, 2], np.uint8)
        pts = C.c_int64(7)

        def refused(rc, words):
            msg = lib.mvk_last_error(hh)
            assert rc != 0 and words in msg, (rc, msg)
            assert all((a == 7).all() for a in out) and pts.value == 7

        refused(lib.mvk_rank(hh, vp, 0, 1, 0, N, *op), b"Q = 0")
        refused(lib.mvk_rank(hh, vp, 4097, 0, 0, N, *op), b"Q = 4097")
        refused(lib.mvk_rank(hh, vp, 3, 0, -1, 5, *op), b"rows [")
        refused(lib.mvk_rank(hh, vp, 3, 0, 1, N, *op), b"rows [")
        refused(lib.mvk_rank(hh, vp, 3, 0, N + 1, 0, *op), b"rows [")
        refused(lib.mvk_rank(hh, None, 3, 0, 0, N, *op), b"NULL")
        for i in range(5):
            refused(lib.mvk_rank(hh, vp, 3, 0, 0, N, *(None if j == i else p for j, p in enumerate(op))), b"NULL")
        refused(lib.mvk_curve(hh, vp, 0, 1, 0, N, C.byref(pts)), b"Q = 0")
        refused(lib.mvk_curve(hh, vp, 2, 0, 0, N, C.byref(pts)), b"ONE ranking")
        refused(lib.mvk_curve(hh, vp, 1, 0, 2, N - 1, C.byref(pts)), b"rows [")
        refused(lib.mvk_curve(hh, None, 1, 0, 0, N, C.byref(pts)), b"NULL")
        refused(lib.mvk_curve(hh, vp, 1, 0, 0, N, None), b"NULL")
        refused(lib.mvk_set_classes(hh, cls2.ctypes.data_as(C.c_void_p), 0, 3), b"cls[2] = 2")
        refused(lib.mvk_set_classes(hh, cls2.ctypes.data_as(C.c_void_p), N - 2, 3), b"rows [")
        refused(lib.mvk_set_classes(hh, None, 0, 3), b"NULL")
        refused(lib.mvk_add(hh, vp, 2 ** 31), b"2^31 - 2")  # (refused before the buffer is looked at)
        refused(lib.mvk_add(hh, vp, -1), b"n = -1")
        refused(lib.mvk_add(hh, None, 3), b"NULL")
        for plan in ((100, 0, 0), (64, 0, 0), (2048, 0, 0), (256, -1, 0), (256, 4097, 0), (256, 0, -1)):
            refused(lib.mvk_test_plan(hh, *plan), b"= ")
        refused(lib.mvk_kernel_ms(hh, None), b"NULL")
        assert lib.mvk_rank(None, vp, 3, 0, 0, N, *op) != 0 and b"index is NULL" in lib.mvk_last_error(None) and all((a == 7).all() for a in out)
        # a refused class value changed nothing, and the index still answers
        assert len(ix) == N
        _compare(ix.rank(np.ascontiguousarray(v[:Q]), bank=True), want, "after the refusals")
        ms = ix.stage_ms()
        assert 0 < ms["total"] < 1e4 and abs(ms["score"] + ms["sort"] + ms["statistics"] - ms["total"]) <= 1e-3 * ms["total"] and min(ms.values()) > 0


def test_a_refusal_is_recorded_by_the_refusing_library_alone(gu, c512):
    """The four kept-corpus libraries open side by side over the same rows: the error text kept_index.h holds (per index, and per thread for the NULL handle) is one
    copy per library — a refusal by one changes no other's, for the open handle or for NULL — and the ranking index answers afterwards as before."""
    from memvul_amd import bank, retrieve

    N, Q = 65, 3
    U, v, Wm = np.ascontiguousarray(c512["U"][:N]), np.ascontiguousarray(c512["V"][:Q]), c512["Wm"]
    cls = _classes("contrast", c512, N, 0)
    vp, wp = v.ctypes.data_as(C.c_void_p), Wm.ctypes.data_as(C.c_void_p)
    with retrieve.ReportIndex(0, 512, Wm, 0) as rx, claims.ClaimIndex(0, 512, Wm, 0) as cx, bank.BankAudit(0, 512, Wm, 0) as bx, _index(c512, 0, N, cls) as kx:
        others = (rx, cx, bx)
        for ix in others:
            ix.add(U)
        for ix in (cx, bx):
            ix.set_classes(cls)

        def texts(ix):
            return ix._fn("last_error")(ix._h), ix._fn("last_error")(None)

        def refuse_create(ix, proj_dim):
            h = C.c_void_p()
            assert ix._fn("create")(0, proj_dim, wp, 0, C.byref(h)) != 0 and not h.value

        # every library holds a text of its own first, under the open handle and under NULL: a copy shared across libraries would show up as another's text
        for i, ix in enumerate(others + (kx,)):
            assert ix._fn("add")(ix._h, None, -1 - i) != 0
            refuse_create(ix, 200 + i)
            assert texts(ix) == (f"n = {-1 - i} rows".encode(), f"proj_dim = {200 + i}: the matcher runs on 512 or 768 features".encode())
        assert len({t for ix in others + (kx,) for t in texts(ix)}) == 8
        before = kx.rank(v, bank=True)
        held = [texts(ix) for ix in others]
        out = [np.full(3 * (Q + 1), 7, np.int64), np.full(Q + 1, 7, np.int64), np.full(Q + 1, 7.0, np.float64), np.full(Q + 1, 7.0, np.float32), np.full(2 * (Q + 1), 7, np.int64)]
        assert kx._fn("rank")(kx._h, vp, 0, 1, 0, N, *(a.ctypes.data_as(C.c_void_p) for a in out)) != 0 and all((a == 7).all() for a in out)
        refuse_create(kx, 100)
        ranks = texts(kx)
        assert ranks == (b"Q = 0: 1 <= Q <= 4096", b"proj_dim = 100: the matcher runs on 512 or 768 features")
        assert [texts(ix) for ix in others] == held
        # and the reverse: a refused claims call
        counts = np.full(Q * 2, 7, np.int64)
        thres = np.full(1, 0.5, np.float32)
        assert cx._fn("counts")(cx._h, vp, Q, thres.ctypes.data_as(C.c_void_p), 0, 0, N, counts.ctypes.data_as(C.c_void_p)) != 0 and (counts == 7).all()
        refuse_create(cx, 300)
        assert texts(cx) == (b"T = 0: 1 <= T <= 64", b"proj_dim = 300: the matcher runs on 512 or 768 features")
        assert texts(kx) == ranks and texts(rx) == held[0] and texts(bx) == held[2]
        after = kx.rank(v, bank=True)
        assert sorted(before) == sorted(after)
        for k in before:
            if isinstance(before[k], np.ndarray):
                _same_bytes(after[k], before[k], f"after the refusals: {k}")
            else:
                assert after[k] == before[k], k
        assert len(kx) == len(rx) == len(cx) == len(bx) == N


# ---- 5: end to end -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_from_a_kept_sweep(gu, c512):
    eng = c512["eng"]
    dims, _ = gu.weights_for(L2, WK)
    n = 200
    ids, lens = synth.make_ids(n, 64, dims.vocab_size, seed=synth.SEED + 77, ragged=True, min_len=3)
    ids[10], lens[10] = ids[3], lens[3]  # one report twice, once in each class: a tie group that holds both
    five = synth.make_ids(5, 64, dims.vocab_size, seed=synth.SEED + 78, ragged=True, min_len=16)
    two = synth.make_ids(2, 64, dims.vocab_size, seed=synth.SEED + 79, ragged=True, min_len=16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = bare_model(eng, c512["Wm"], 5)
        arrays = {"type": "test", "ids": ids, "lens": lens, "same": np.zeros(n, bool), "urls": [f"https://example.invalid/issues/{i}" for i in range(n)]}
        # the witness first: the engine's own P(same) of the reports against the bank of five and against the bank of seven
        eng.anchor_reset()
        eng.anchor_append(*five)
        m.sweep_arrays(arrays, batch_size=64, with_probs=True, keep=True)
        ps5 = m.rematch_arrays(arrays, with_probs=True)[2]
        eng.anchor_append(*two)
        m._golden_labels = [f"CWE-{i}" for i in range(7)]
        ps7 = m.rematch_arrays(arrays, with_probs=True)[2]
        assert ps5.dtype == ps7.dtype == np.float32 and ps5.shape == (n, 5) and ps7.shape == (n, 7) and ps7[:, :5].tobytes() == ps5.tobytes()
        same = (ps5[:, 0] > np.median(ps5[:, 0])) ^ (np.random.default_rng(9).random(n) < 0.1)  # informative for anchor 0
        same[3], same[10] = True, False
        # the rankings to compare — five anchors, seven after the bank was edited, seven against the opposite classes (every AUC crosses one half) — and the
        # fixture conditions on the reference alone
        runs = [(False, 0, ps5), (False, 2, ps7), (True, 0, ps7)]
        exacts = [[kit.reference_rank(col, ~same if flipped else same) for col in [ps[:, g] for g in range(ps.shape[1])] + [kit.bank_scores(ps)]] for flipped, _, ps in runs]
        bite = _Bite()
        for exact in exacts:
            bite.see(exact)
        bite.check()
        eng.anchor_reset()
        eng.anchor_append(*five)
        m._golden_labels = [f"CWE-{i}" for i in range(5)]
        for (flipped, more, ps), exact in zip(runs, exacts):
            if not more:
                arrays["same"] = ~same if flipped else same
                m.sweep_arrays(arrays, batch_size=64, with_probs=True, keep=True)
            else:  # the bank is edited, the corpus is not encoded again and the index is not refilled
                eng.anchor_append(*two)
            m._golden_labels = [f"CWE-{i}" for i in range(ps.shape[1])]
            index = m._kept.indexes["ranking"]
            assert m.rematch_arrays(arrays, with_probs=True)[2].tobytes() == ps.tobytes()  # the witness is what the engine gives now
            out = m.anchor_ranking(arrays)
            assert (more == 0 and index is None) or m._kept.indexes["ranking"] is index
            assert [e["anchor"] for e in out] == m._golden_labels + ["bank"]
            for e, x in zip(out, exact):
                tp, fp = x["best"]
                assert (e["n_neg"], e["n_pos"], e["n_nan"]) == x["n"] and e["auc"] == rank.auc_of(x["u2"], x["n"][1], x["n"][0])
                assert e["best_thres"] == float(x["best_thres"]) and (e["best_positives"], e["best_claimed"]) == (tp, tp + fp) and e["best_f1"] == 2 * tp / (tp + fp + x["n"][1])
                assert abs(Fraction(e["ap"]) - x["ap"]) <= kit.ap_bound(x)
            gu.record("rank_end_to_end", anchors=len(out) - 1, auc=[e["auc"] for e in out], best_f1=[e["best_f1"] for e in out])
        ranking = m._kept.indexes["ranking"]
        assert ranking is not None and m._kept.indexes == dict(reports=None, claims=None, bank=None, ranking=ranking)
        m._kept.drop()
        assert m._kept.indexes == dict.fromkeys(("reports", "claims", "bank", "ranking"))
