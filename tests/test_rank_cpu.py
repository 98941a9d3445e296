"""Per-anchor ranking quality (memvul_amd/rank.py, libmemvul_rank.so): what needs no GPU — the names, the build, the built kernels' resources, the definitions against
sklearn, the plan in numpy against the definitions (and the faults it must see), the Python validation on a recording stub, and ModelMemory.anchor_ranking / the
command line on the oracle-backed stand-in."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from memvul_amd import bank, binding, build, claims, custom_metric, rank, retrieve

import kept_index_kit as kk
import plumbing_util as pu
import rank_kit as kit
from kept_index_kit import _CountingEngine, _KeepingEngine, _NumpyBank, _NumpyClaims, _NumpyIndex, _NumpyKept, _inputs, standin_model  # noqa: F401  (standin_model is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memvul_amd", "csrc")
NEW_KERNELS = ("rank_weight_delta_kernel", "rank_row_term_kernel", "rank_vector_prep_kernel", "rank_score_kernel", "rank_bank_fold_kernel", "rank_hist_kernel",
               "rank_digit_scan_kernel", "rank_scatter_kernel", "rank_tile_sums_kernel", "rank_tile_scan_kernel", "rank_stats_kernel", "rank_finish_kernel")
W512 = kk.W512


@pytest.fixture(scope="module")
def libs():
    return build.build_all(verbose=False)


# ---- the names and the exception rule -----------------------------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "memvul_rank.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(libs):
    declared = sorted(set(re.findall(r"\b(mvk_[a-z_0-9]+)\s*\(", _header())))
    assert declared == sorted(rank.RANK_SYMBOLS) and len(declared) == 12
    lib = rank.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libmemvul_rank.so does not export {name}"
    exported = subprocess.run([kit.llvm_tool("llvm-readelf"), "--dyn-syms", build.LIB_PATH_RANK], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mvk_\w+)", exported))) == declared
    assert not re.search(r"\bmv[rcb]?_[a-z]", exported)  # no mv_, mvr_, mvc_ or mvb_ name
    raw = open(os.path.join(ROOT, "include", "memvul_rank.h")).read()
    macros = dict(re.findall(r"#define (MVK_MAX_\w+) \(?([0-9l< ]+)\)?", raw))
    assert macros["MVK_MAX_VECTORS"].strip() == "4096" == str(rank.MAX_VECTORS) and int(macros["MVK_MAX_ROWS"].strip("l ")) == rank.MAX_ROWS
    assert macros["MVK_MAX_RANK_ROWS"].strip() == "1ll << 26" and rank.MAX_RANK_ROWS == 1 << 26
    assert rank.MAX_RANK_ROWS ** 2 // 2 < 2 ** 63  # u2 fits int64
    others = set(claims.CLAIMS_SYMBOLS) | set(retrieve.RETRIEVE_SYMBOLS) | set(bank.BANK_SYMBOLS)
    assert not set(rank.RANK_SYMBOLS) & others and not hasattr(binding, "RANK_SYMBOLS")


def test_no_cpp_exception_can_cross_the_boundary():
    src = open(os.path.join(CSRC, "rank.hip")).read()
    heads = re.findall(r"^int (mvk_\w+)\(([^{;]*?)\)\s*(try\s*)?\{", src, flags=re.M)
    declared = sorted(set(re.findall(r"^\s*int\s+(mvk_\w+)\s*\(", _header(), flags=re.M)))
    assert len(declared) == 9 and sorted(name for name, _, _ in heads) == declared
    assert all(guard for _, _, guard in heads), [name for name, _, guard in heads if not guard]
    assert src.count("catch (...) { return on_exception(") == len(heads)


# ---- the build ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_build_all_leaves_six_fresh_libraries_and_returns_two_paths(libs):
    assert list(libs) == [build.LIB_PATH, build.LIB_PATH_DEV]
    assert not build.is_stale() and not build.is_stale(dev=True) and not build.tok_is_stale() and not build.retrieve_is_stale() and not build.claims_is_stale()
    assert not build.bank_is_stale() and not build.rank_is_stale()
    assert os.path.exists(build.LIB_PATH_RANK) and os.path.basename(build.LIB_PATH_RANK) == build.RANK_LIB_NAME == "libmemvul_rank.so"
    assert rank.LIB_PATH == build.LIB_PATH_RANK and build.build_rank(verbose=False) == build.LIB_PATH_RANK
    needed = subprocess.run([kit.llvm_tool("llvm-readelf"), "-d", build.LIB_PATH_RANK], capture_output=True, text=True, check=True).stdout
    assert "libmemvul" not in "".join(ln for ln in needed.splitlines() if "NEEDED" in ln)  # it links against nothing of this tree
    for other in (build.LIB_PATH, build.LIB_PATH_DEV, build.LIB_PATH_TOK, build.LIB_PATH_RETRIEVE, build.LIB_PATH_CLAIMS, build.LIB_PATH_BANK):  # and nothing against it
        needed = subprocess.run([kit.llvm_tool("llvm-readelf"), "-d", other], capture_output=True, text=True, check=True).stdout
        assert "libmemvul_rank" not in needed, other


def test_the_kernels_are_the_recorded_ones(libs):
    kk.check_kernels_are_the_recorded_ones(build.LIB_PATH_RANK, "rank")


def test_the_module_prints_the_new_path_after_the_bank(libs):
    src = open(os.path.join(ROOT, "memvul_amd", "build.py")).read()
    assert re.search(r'__name__ == "__main__":\n\s+print\(.*LIB_PATH_BANK, LIB_PATH_RANK\]', src)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "rank_is_stale()" in entry and "rank.load_library()" in entry


def _plain_name(mangled: str) -> str:
    """The function name inside an Itanium-mangled kernel symbol (_Z<length><name>...); an unmangled symbol as it is, without the descriptor's suffix."""
    m = re.match(r"_Z(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled.removesuffix(".kd")


def test_the_other_libraries_do_not_know_the_new_files(libs, monkeypatch):
    assert build.SIDE_LIBS["rank"] == (build.RANK_LIB_NAME, build.RANK_SOURCES, build.RANK_HEADERS)
    new = [os.path.join(CSRC, "rank.hip"), os.path.join(CSRC, "rank_sort.h"), os.path.join(ROOT, "include", "memvul_rank.h")]
    assert kk.opened_by_fingerprint(monkeypatch, *build.SIDE_LIBS["rank"][1:]) == set(new) | {os.path.join(CSRC, h) for h in kk.KEPT_SHARED}
    kk.check_the_shared_headers_belong_to_the_four_kept_libraries(monkeypatch)
    kk.check_the_index_plumbing_is_defined_once()
    opened = kk.opened_by_fingerprint(monkeypatch)
    for other in ("tok", "retrieve", "claims", "bank"):
        opened |= kk.opened_by_fingerprint(monkeypatch, *build.SIDE_LIBS[other][1:])
    assert not opened & set(new)
    for name in os.listdir(CSRC):  # nothing any other library is built from includes the new header, and the new files include none of theirs but the two shared ones
        if name not in ("rank.hip", "rank_sort.h"):
            text = open(os.path.join(CSRC, name)).read()
            assert "rank_sort.h" not in text and "memvul_rank.h" not in text, name
    src = open(os.path.join(CSRC, "rank.hip")).read() + open(os.path.join(CSRC, "rank_sort.h")).read()
    assert sorted(re.findall(r'#include\s+"([^"]+)"', src)) == sorted(["../../include/memvul_rank.h", "rank_sort.h", "kept_index.h", "kept_terms.h"])
    for theirs in ("claim_sweep.h", "bank_cover.h", "report_topk.h", "match_topk.h", "memvul_claims.h", "memvul_bank.h", "memvul_retrieve.h"):
        assert theirs not in src, theirs
    new_map = build.kernel_fingerprints(build.LIB_PATH_RANK)
    kernels = [k for k in new_map if k.endswith(".kd")]
    for n in NEW_KERNELS:
        assert any(n in k for k in kernels), n
    assert all(re.match(r"_Z\d+rank_", k) for k in kernels), kernels  # every kernel's name starts with rank_
    for other in (build.LIB_PATH, build.LIB_PATH_TOK, build.LIB_PATH_RETRIEVE, build.LIB_PATH_CLAIMS, build.LIB_PATH_BANK):
        other_map = build.kernel_fingerprints(other)
        assert other_map and not set(new_map) & set(other_map), other
        assert not [k for k in other_map if any(n in k for n in NEW_KERNELS)], other
        theirs = {_plain_name(k) for k in other_map if k.endswith(".kd")}  # and no kernel name of the new library contains one of theirs
        assert theirs and not [(k, t) for k in kernels for t in theirs if t in k], other


def test_no_kernel_uses_scratch_or_spills_and_lds_stays_within_the_cu(libs, tmp_path):
    (co,) = build.device_code_objects(build.LIB_PATH_RANK)
    elf = tmp_path / "gfx950.co"
    elf.write_bytes(co)
    notes = subprocess.run([kit.llvm_tool("llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes):
        name = re.search(r"\.name:\s+(\S+)", blk)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        if name and scratch and lds:
            kernels[name.group(1)] = (int(scratch.group(1)), int(lds.group(1)), int(spill.group(1)) if spill else 0)
    for n in NEW_KERNELS:
        assert any(n in k for k in kernels), n
    assert len([k for k in kernels if "rank_score_kernel" in k]) == 2  # P 512 / 768
    assert len([k for k in kernels if "rank_stats_kernel" in k]) == 6  # 256 / 512 / 1 024 rows per tile x with and without the curve
    assert len(kernels) == 28
    for k, (scratch, lds, spill) in kernels.items():
        assert scratch == 0 and spill == 0 and lds <= 160 * 1024, (k, scratch, lds, spill)


# ---- the definitions against sklearn ----------------------------------------------------------------------------------------------------------------------------------

PREFIXES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099)


@pytest.fixture(scope="module")
def oracle_scores():
    """P(same) of the fixtures of the GPU file through the oracle's matcher: {(P, same_idx): fp32 [N, Q]}, and the classes (random at 0.3)."""
    from oracle import memvul_oracle as orc

    out = {}
    for P, N, Q in ((512, 4099, 33), (768, 1000, 124)):
        U, V, W = kit.rkit.fixture(43 + P, N, P, Q, block_rows=64)
        _, p, _, _ = orc.match(U, V, W, 0)
        for same_idx in (0, 1):
            out[P, same_idx] = np.ascontiguousarray(p[:, :, same_idx].astype(np.float32))
    cls = (np.random.default_rng(3).random(4099) < 0.3).astype(np.uint8)
    return out, cls


@pytest.mark.parametrize("P,same_idx", [(512, 0), (512, 1), (768, 0), (768, 1)])
def test_the_definitions_are_sklearns(oracle_scores, P, same_idx):
    from sklearn import metrics

    ps, cls = oracle_scores[0][P, same_idx], oracle_scores[1]
    mixed, compared, worst = 0, 0, 0.0
    for q in range(0, ps.shape[1], 4 if P == 512 else 17):
        for n in [n for n in PREFIXES if n <= len(ps)]:
            p, c = ps[:n, q], cls[:n]
            e = kit.reference_rank(p, c)
            assert e["n"] == (int((c == 0).sum()), int(c.sum()), 0)
            auc = rank.auc_of(e["u2"], e["n"][1], e["n"][0])
            if auc is None:
                assert e["n"][0] == 0 or e["n"][1] == 0
                continue
            fpr, tpr, _ = metrics.roc_curve(c, p.astype(np.float64), pos_label=1, drop_intermediate=False)
            want = (metrics.auc(fpr, tpr), metrics.average_precision_score(c, p.astype(np.float64), pos_label=1))
            assert want == pytest.approx(custom_metric.roc_auc_ap(c, p.astype(np.float64)), abs=1e-12)  # (what the package's own metric calls)
            worst = max(worst, abs(auc - want[0]), abs(float(e["ap"]) - want[1]))
            assert abs(auc - want[0]) <= 1e-12 and abs(float(e["ap"]) - want[1]) <= 1e-12, (q, n, auc, float(e["ap"]), want)
            thres, tp, fp = kit.reference_curve(p, c)
            assert np.array_equal(tp / e["n"][1], tpr[1:]) and np.array_equal(fp / e["n"][0], fpr[1:]) and len(thres) == e["groups"]
            mixed += e["mixed"]
            compared += 1
    print(f"P={P} same_idx={same_idx}: {compared} rankings compared, {mixed} mixed-class tie groups, largest distance {worst:.3g}")
    assert compared >= 40 and mixed >= 2  # the fixture's duplicate rows tie across classes


def test_the_best_cut_by_hand():
    """pos 0.9, neg 0.8, neg 0.75, pos 0.7: F1 = 2/3 at 0.9 and at 0.7 — the highest threshold wins; the degenerate cases."""
    p, c = np.array([0.7, 0.9, 0.8, 0.75], np.float32), np.array([1, 1, 0, 0], np.uint8)
    e = kit.reference_rank(p, c)
    assert e["best_thres"] == np.float32(0.9) and e["best"] == (1, 0) and e["f1_ties"] == 1 and e["u2"] == 4 and e["ap"] == Fraction(1, 2) * 1 + Fraction(1, 2) * Fraction(2, 4)
    e = kit.reference_rank(p, np.zeros(4, np.uint8))
    assert e["u2"] == 0 and e["ap"] is None and np.isnan(e["best_thres"]) and e["best"] == (0, 0) and e["n"] == (4, 0, 0)
    e = kit.reference_rank(p, np.ones(4, np.uint8))
    assert e["u2"] == 0 and e["ap"] == 1 and e["best_thres"] == np.float32(0.7) and e["best"] == (4, 0)
    e = kit.reference_rank(np.array([0.5, 0.5, 0.5], np.float32), np.array([1, 0, 0], np.uint8))  # one tie group: every pair is a tie
    assert e["u2"] == 2 and rank.auc_of(e["u2"], 1, 2) == 0.5 and e["ap"] == Fraction(1, 3) and e["groups"] == 1 and e["mixed"] == 1
    e = kit.reference_rank(np.array([0.5, np.nan, 0.25], np.float32), np.array([1, 1, 0], np.uint8))
    assert e["n"] == (1, 1, 1) and e["u2"] == 2
    assert np.array_equal(kit.bank_scores(np.array([[0.1, 0.9], [np.nan, 0.2]], np.float32)), np.array([0.9, np.nan], np.float32), equal_nan=True)


# ---- the plan in numpy ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tie_heavy():
    """P(same) [4099] of the fixture's first vector, quantised to 1/64 (tie groups that hold both classes and cross tile edges), with a NaN row; a class assignment
    that follows the score, 10 % flipped; and, on top, the hand-made F1 tie in a second column."""
    U, V, W = kit.rkit.fixture(11, 4099, 64, 3)
    p = (np.round(kit.rkit.psame_f64(U, V, W, 0)[:, 0] * 64) / 64).astype(np.float32)
    p[1234] = np.float32("nan")
    rng = np.random.default_rng(5)
    cls = ((p > np.nanmedian(p)) ^ (rng.random(4099) < 0.1)).astype(np.uint8)
    p.setflags(write=False)
    return p, cls


def _same(got, want):
    bad = [k for k in ("n", "u2", "best") if got[k] != want[k]]
    if np.float32(got["best_thres"]).tobytes() != np.float32(want["best_thres"]).tobytes():
        bad.append("best_thres")
    if want["ap"] is None:
        if not np.isnan(got["ap"]):
            bad.append("ap")
    elif not abs(Fraction(got["ap"]) - want["ap"]) <= kit.ap_bound(want):
        bad.append("ap")
    return bad


@pytest.mark.parametrize("tile", [256, 512, 1024])
def test_the_plan_gives_the_definitions(tie_heavy, tile):
    p, cls = tie_heavy
    aps = {}
    for first, count in ((0, 4099), (0, 1), (0, 2), (63, 130), (65, 64), (1, 255), (0, 256), (3, 257), (1000, 1000), (1230, 10), (5, 0)):
        want = kit.reference_rank(p[first:first + count], cls[first:first + count])
        got = kit.plan_rank(p, cls, first, count, tile)
        assert _same(got, want) == [], (first, count, got, want)
        aps[first, count] = got["ap"]
    for kind in (np.zeros, np.ones):  # one class only
        c = kind(4099, np.uint8)
        assert _same(kit.plan_rank(p, c, 0, 4099, tile), kit.reference_rank(p, c)) == []
    if tile != 256:  # ap: the same bits whatever the tile
        for (first, count), ap in aps.items():
            other = kit.plan_rank(p, cls, first, count, 256)["ap"]
            assert np.float64(ap).tobytes() == np.float64(other).tobytes(), (first, count)


@pytest.mark.parametrize("fault", kit.FAULTS)
def test_the_plan_model_sees_each_seeded_fault(tie_heavy, fault):
    p, cls = tie_heavy
    first, count, tile = 63, 4000, 256
    if fault == "f1_low":  # two thresholds of equal best F1
        p, cls, first, count = np.array([0.7, 0.9, 0.8, 0.75], np.float32), np.array([1, 1, 0, 0], np.uint8), 0, 4
    want = kit.reference_rank(p[first:first + count], cls[first:first + count])
    # the fixture contains what the fault needs, shown on the reference alone
    thres, tp, fp, TP, FP, _ = kit._groups(p[first:first + count], cls[first:first + count])
    if fault == "tie_win":
        assert want["mixed"] >= 1
    if fault == "tie_cut":  # a tie group crossing a tile edge: its rows in the ascending order straddle a multiple of the tile
        M = want["n"][0] + want["n"][1]
        lo = M - (TP + FP)  # the group's first position, ascending
        hi = lo + tp + fp - 1
        assert ((lo // tile) != (hi // tile)).any()
    if fault == "f1_low":
        assert want["f1_ties"] >= 1
    if fault == "nan_ranked":
        assert want["n"][2] == 1
    if fault in ("local_class", "first_dropped"):
        assert not np.array_equal(cls[first:first + count], cls[:count]) and not np.array_equal(cls[first:first + count], cls[first + np.arange(count) % 256])
    assert _same(kit.plan_rank(p, cls, first, count, tile), want) == []
    seen = _same(kit.plan_rank(p, cls, first, count, tile, fault=fault), want)
    assert seen, fault
    must = {"tie_win": {"u2"}, "unstable": {"u2"}, "tie_cut": {"u2"}, "f1_low": {"best_thres", "best"}, "nan_ranked": {"n"}, "local_class": {"n", "u2"},
            "first_dropped": {"u2"}}[fault]
    assert must <= set(seen), (fault, seen)


# ---- validation before any library call --------------------------------------------------------------------------------------------------------------------------------

class _StubLib(kk.StubLib):
    PREFIX = "mvk_"
    points = 3

    def rank(self, h, v, Q, bank, first, count, n, u2, ap, best_thres, best):
        self.log.append(("rank", Q, bank, first, count))
        S = Q + bank
        np.ctypeslib.as_array(C.cast(n, C.POINTER(C.c_int64)), (S, 3))[:] = [[5, 2, 1]] * S
        np.ctypeslib.as_array(C.cast(u2, C.POINTER(C.c_int64)), (S,))[:] = 15
        np.ctypeslib.as_array(C.cast(ap, C.POINTER(C.c_double)), (S,))[:] = 0.75
        np.ctypeslib.as_array(C.cast(best_thres, C.POINTER(C.c_float)), (S,))[:] = 0.5
        np.ctypeslib.as_array(C.cast(best, C.POINTER(C.c_int64)), (S, 2))[:] = [[2, 1]] * S
        return 0

    def curve(self, h, v, Q, bank, first, count, points):
        self.log.append(("curve", Q, bank, first, count))
        C.cast(points, C.POINTER(C.c_int64))[0] = self.points
        return 0

    def fetch(self, h, thres, tp, fp):
        self.log.append(("fetch",))
        return 0


def test_bad_arguments_raise_before_any_call():
    lib = _StubLib()
    for args in ((0, 500, W512, 0), (0, 512, W512, 2), (0, 512, W512[:, :100], 0), (0, 512, W512.astype(np.float64), 0), (-1, 512, W512, 0), (0, 512.0, W512, 0)):
        with pytest.raises((ValueError, TypeError)):
            rank.RankIndex(*args, lib=lib)
    assert lib.log == []
    with rank.RankIndex(0, 512, W512, 1, lib=lib) as ix:
        assert lib.log == [("create", 0, 512, 1)]
        ok = np.zeros((10, 512), np.float32)
        for bad in (ok.astype(np.float64), ok[:, :500], ok[:, ::2], ok.tolist(), ok[0]):
            with pytest.raises((ValueError, TypeError)):
                ix.add(bad)
        ix.add(ok)
        assert lib.log[-1] == ("add", 10) and len(ix) == 10
        v = np.zeros((3, 512), np.float32)
        n_calls = len(lib.log)
        with pytest.raises(RuntimeError, match="no curve is held"):
            ix.fetch()
        calls = (lambda: ix.rank(v, 3, 8), lambda: ix.rank(v, -1), lambda: ix.rank(v[:0]), lambda: ix.rank(v.astype(np.float64)), lambda: ix.rank(v, bank=1),
                 lambda: ix.rank(v, 0.0), lambda: ix.rank(np.zeros((4097, 512), np.float32)), lambda: ix.rank(np.zeros((3, 768), np.float32)), lambda: ix.rank(v.tolist()),
                 lambda: ix.curve(v), lambda: ix.curve(v, bank="yes"), lambda: ix.curve(v[:1], False, 5, 6), lambda: ix.curve(v[:1].astype(np.float16)),
                 lambda: ix.set_classes(np.zeros(11, np.uint8)), lambda: ix.set_classes(np.full(3, 2, np.uint8)), lambda: ix.set_classes(np.zeros(3, np.int64)),
                 lambda: ix.set_classes([0, 1]), lambda: ix.set_classes(np.zeros(3, np.uint8), -1))
        for i, call in enumerate(calls):
            with pytest.raises((ValueError, TypeError)):
                call()
            assert len(lib.log) == n_calls, i
        out = ix.rank(v, 2, bank=True)
        assert lib.log[-1] == ("rank", 3, 1, 2, 8) and out["n"].shape == (4, 3) and out["u2"].dtype == np.int64 and out["ap"].dtype == np.float64
        assert out["best_thres"].dtype == np.float32 and out["best"].shape == (4, 2) and out["auc"] == [15 / 20] * 4
        assert ix.rank(v)["n"].shape == (3, 3) and lib.log[-1] == ("rank", 3, 0, 0, 10)
        entries = rank.format_ranking(["a", "b", "c"], out)
        assert [e["anchor"] for e in entries] == ["a", "b", "c", "bank"] and set(entries[0]) == {"anchor", "n_pos", "n_neg", "n_nan", "auc", "ap", "best_thres", "best_f1",
                                                                                              "best_claimed", "best_positives"}
        assert entries[3] == dict(anchor="bank", n_pos=2, n_neg=5, n_nan=1, auc=0.75, ap=0.75, best_thres=0.5, best_f1=2 * 2 / (2 + 1 + 2), best_claimed=3, best_positives=2)
        json.dumps(entries)
        with pytest.raises(ValueError):
            rank.format_ranking(["a"], out)
        # the held curve
        thres, tp, fp = ix.curve(v, bank=True, first=1)
        assert lib.log[-2:] == [("curve", 3, 1, 1, 9), ("fetch",)] and thres.shape == tp.shape == fp.shape == (3,) and thres.dtype == np.float32 and tp.dtype == fp.dtype == np.int64
        ix.curve(v[:1])
        assert lib.log[-2] == ("curve", 1, 0, 0, 10)
        ix.fetch()  # as often as asked
        assert len(ix) == 10  # (count leaves it alone)
        ix.fetch()
        for drop in (lambda: ix.set_classes(np.array([True, False, True]), 7), lambda: ix.test_plan(256, 5, 1 << 20), lambda: ix.rank(v), lambda: ix.add(ok), lambda: ix.reset()):
            ix.curve(v[:1])
            drop()
            with pytest.raises(RuntimeError, match="no curve is held"):
                ix.fetch()
        assert ("classes", 7, 3) in lib.log and ("plan", 256, 5, 1 << 20) in lib.log and len(ix) == 0
        with pytest.raises(RuntimeError, match="stub"):
            ix.kernel_ms()
    assert lib.log[-1] == ("destroy",)
    with pytest.raises(RuntimeError, match="closed"):
        ix.rank(v)
    assert rank.auc_of(3, 0, 5) is None and rank.auc_of(3, 5, 0) is None and rank.auc_of(2 ** 62, 2 ** 31, 2 ** 31) == 0.5


# ---- ModelMemory.anchor_ranking and the command line on the stand-in -----------------------------------------------------------------------------------------------------

class _NumpyRank(_NumpyKept):
    """P(same) met with the definitions of rank_kit."""
    made = []

    def rank(self, v, first=0, count=None, bank=False):
        count = len(self.u) - first if count is None else count
        ps, cls = self._p(v)[first:first + count], self.cls[first:first + count]
        out = kit.reference_matrix(ps, cls, bank)
        out["ap"] = np.array([float("nan") if e["ap"] is None else float(e["ap"]) for e in out["exact"]], np.float64)
        out["auc"] = [rank.auc_of(u, n[1], n[0]) for u, n in zip(out["u2"].tolist(), out["n"].tolist())]
        return out

    def curve(self, v, bank=False, first=0, count=None):
        ps = self._p(v)
        return kit.reference_curve(kit.bank_scores(ps) if bank else ps[:, 0], self.cls)


def _check_entries(entries, ps, same, labels, bank=True):
    from sklearn import metrics

    assert [e["anchor"] for e in entries] == list(labels) + (["bank"] if bank else [])
    cols = [ps[:, g] for g in range(ps.shape[1])] + ([ps.max(1)] if bank else [])
    for e, col in zip(entries, cols):
        want = kit.reference_rank(col, same)
        assert (e["n_neg"], e["n_pos"], e["n_nan"]) == want["n"] == (int((~same).sum()), int(same.sum()), 0)
        if not same.any():  # nothing to rank for: every figure is undefined
            assert (e["auc"], e["ap"], e["best_thres"], e["best_f1"], e["best_claimed"], e["best_positives"]) == (None, None, None, None, 0, 0)
            continue
        assert e["auc"] == rank.auc_of(want["u2"], want["n"][1], want["n"][0]) and e["ap"] == float(want["ap"]) and e["best_thres"] == float(want["best_thres"])
        tp, fp = want["best"]
        assert e["best_positives"] == tp and e["best_claimed"] == tp + fp and e["best_f1"] == 2 * tp / (tp + fp + want["n"][1])
        pred = col >= np.float32(e["best_thres"])
        assert (int((pred & same).sum()), int((pred & ~same).sum())) == (tp, fp)
        assert e["best_f1"] == pytest.approx(metrics.f1_score(same, pred)) and e["best_f1"] >= max(metrics.f1_score(same, col >= t) for t in col) - 1e-12
    return cols


def test_anchor_ranking_on_the_standin(standin_model):
    model, arrays, fx = standin_model
    best, _, ps = model.sweep_arrays(arrays, batch_size=8, with_probs=True, keep=True)
    ps = ps.astype(np.float32)
    same = np.asarray(arrays["same"], bool)
    assert 0 < same.sum() < len(same)
    entries = model.anchor_ranking(arrays, index_factory=_NumpyRank)
    ix = _NumpyRank.made[0]
    pm = ix._p(model.engine.anchor_get())  # the stand-in's own matrix: the oracle's matcher on the kept embeddings (the sweep's agrees to an fp32 step)
    assert np.abs(pm - ps).max() <= 2e-7
    _check_entries(entries, pm, same, model._golden_labels)
    # the bank entry is what the reference's own metric measures on the sweep's best scores
    auc, ap = custom_metric.roc_auc_ap(same.astype(np.int64), np.asarray(best[:, model._same_idx], np.float64))
    assert abs(entries[-1]["auc"] - auc) <= 1e-12 and abs(entries[-1]["ap"] - ap) <= 1e-12
    json.dumps(entries)
    assert len(_NumpyRank.made) == 1 and np.array_equal(ix.w, fx[4]["_projector.weight"]) and ix.u.shape == (23, 512) and np.array_equal(ix.cls, same.astype(np.uint8))
    # the index lives beside the three, which keep their keys; the same object serves the next call; one download serves all four
    assert model._kept.indexes == dict(reports=None, claims=None, bank=None, ranking=ix) and model._kept.indexes["ranking"] is ix and _CountingEngine.downloads == 1
    assert model._kept.embed is not None  # (this index never releases the host copy)
    two = np.ascontiguousarray(model.engine.anchor_get()[[2, 0]])
    no_bank = model.anchor_ranking(arrays, vectors=two, labels=["x", "y"], bank=False, index_factory=_NumpyRank)
    assert len(_NumpyRank.made) == 1
    _check_entries(no_bank, ix._p(two), same, ["x", "y"], bank=False)  # (the oracle's matrix product is not the same to the bit for another set of vectors)
    model.anchor_claims(arrays, 0.5, index_factory=_NumpyClaims)
    model.anchor_reports(arrays, 3, index_factory=_NumpyIndex)
    assert _CountingEngine.downloads == 1 and model._kept.embed is None
    with pytest.raises(ValueError):
        model.anchor_ranking(arrays, vectors=model.engine.anchor_get(), labels=["one"], index_factory=_NumpyRank)
    # a new sweep drops the index with the other three
    model.sweep_arrays(arrays, 4, 20, batch_size=8, with_probs=True, keep=True)
    assert ix.closed and model._kept.indexes["ranking"] is None and set(model._kept.indexes) == {"reports", "claims", "bank", "ranking"}
    with pytest.raises(RuntimeError, match="no kept sweep"):
        model.anchor_ranking(arrays, index_factory=_NumpyRank)
    part = model.anchor_ranking(arrays, 4, 20, index_factory=_NumpyRank)
    assert len(_NumpyRank.made) == 2 and _NumpyRank.made[1].u.shape == (16, 512) and np.array_equal(_NumpyRank.made[1].cls, same[4:20].astype(np.uint8))
    _check_entries(part, pm[4:20], same[4:20], model._golden_labels)
    model._kept.drop()
    assert _NumpyRank.made[1].closed and model._kept.indexes["ranking"] is None


def test_the_command_line(capsys, tmp_path):
    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=12, n_anchors=4, layers=2)
    try:
        _KeepingEngine.created, _NumpyRank.made, _NumpyBank.made = [], [], []
        out, tf, cf = tmp_path / "rank.jsonl", tmp_path / "thres.json", tmp_path / "curve.json"
        std = ["--archive", arch, "--golden", golden, "--input", test_path]
        rc = rank.main(std + ["--out", str(out), "--thres-file-out", str(tf), "--curve", "bank", "--curve-out", str(cf)], engine_factory=_KeepingEngine, index_factory=_NumpyRank)
        entries = [json.loads(ln) for ln in open(out)]
        assert rc == 0 and capsys.readouterr().out.strip() == "" and _NumpyRank.made[0].closed
        eng = _KeepingEngine.created[0]
        ids, lens, _ = _inputs(arch, golden, test_path)
        ps = _NumpyRank.made[0]._p(eng.anchor_get())
        assert np.abs(ps - eng.forward(ids, lens)["probs"][:, :, 0]).max() <= 2e-7
        same = _NumpyRank.made[0].cls.astype(bool)
        labels = [f"CWE-{100 + i}" for i in range(4)]
        cols = _check_entries(entries, ps, same, labels)
        per = json.load(open(tf))
        assert per == {e["anchor"]: e["best_thres"] for e in entries[:4]}
        curve = json.load(open(cf))
        thres, tp, fp = kit.reference_curve(cols[-1], same)
        assert curve == {"anchor": "bank", "thres": [float(x) for x in thres], "tp": tp.tolist(), "fp": fp.tolist()}
        # the thresholds file is what the bank audit's command line reads
        rc = bank.main(std + ["--thres-file", str(tf)], engine_factory=_KeepingEngine, index_factory=_NumpyBank)
        doc = json.loads(capsys.readouterr().out)
        assert rc == 0 and [a["thres"] for a in doc["anchors"]] == [per[a] for a in labels]
        for a, e in zip(doc["anchors"], entries):  # at its best threshold an anchor claims what the ranking said
            assert a["claimed"] == [e["best_claimed"] - e["best_positives"], e["best_positives"]]
        rc = rank.main(std + ["--anchors", "CWE-102,CWE-100", "--no-bank", "--curve", "CWE-100", "--curve-out", str(cf)], engine_factory=_KeepingEngine, index_factory=_NumpyRank)
        two = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines()]
        ps2 = _NumpyRank.made[-1]._p(np.ascontiguousarray(eng.anchor_get()[[2, 0]]))
        assert rc == 0
        _check_entries(two, ps2, same, ["CWE-102", "CWE-100"], bank=False)
        thres, tp, fp = kit.reference_curve(_NumpyRank.made[-1]._p(np.ascontiguousarray(eng.anchor_get()[:1]))[:, 0], same)
        assert json.load(open(cf)) == {"anchor": "CWE-100", "thres": [float(x) for x in thres], "tp": tp.tolist(), "fp": fp.tolist()}
        for bad in (["--curve", "bank"], ["--curve-out", str(cf)], ["--curve", "CWE-999", "--curve-out", str(cf)], ["--anchors", "CWE-999"]):
            with pytest.raises(SystemExit):
                rank.main(std + bad, engine_factory=_KeepingEngine, index_factory=_NumpyRank)
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- no GPU, no index -------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_constructor_raises_without_a_gpu(libs):
    try:
        has_gpu = subprocess.run(["/opt/rocm/bin/rocm_agent_enumerator"], capture_output=True, text=True).stdout.count("gfx9") > 0
    except Exception:
        has_gpu = False
    with pytest.raises(RuntimeError, match="mvk_create"):
        rank.RankIndex(4096 if has_gpu else 0, 512, W512, 0)  # (with a GPU: a device that is not there)
    with pytest.raises(RuntimeError, match="not found"):
        rank.load_library(os.path.join(ROOT, "memvul_amd", "lib", "no_such_library.so"))
