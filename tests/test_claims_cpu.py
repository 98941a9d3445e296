"""Per-anchor claims (memvul_amd/claims.py, libmemvul_claims.so): what needs no GPU — the names, the build, the built kernels' resources, the plan in numpy against
the rule it must reproduce (and the faults it must see), the rounding-up rule for float64 thresholds, the Python validation on a recording stub, and
ModelMemory.anchor_claims / the command line on the oracle-backed stand-in."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from memvul_amd import binding, build, claims, retrieve

import claims_kit as kit
import kept_index_kit as kk
import plumbing_util as pu
from kept_index_kit import _CountingEngine, _KeepingEngine, _NumpyClaims, _NumpyIndex, _inputs, standin_model  # noqa: F401  (standin_model is a fixture)
from test_f32_form_cpu import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memvul_amd", "csrc")
NEW_KERNELS = ("claim_weight_delta_kernel", "claim_row_term_kernel", "claim_vector_prep_kernel", "claim_score_kernel", "claim_fold_kernel", "claim_scan_kernel")


@pytest.fixture(scope="module")
def libs():
    return build.build_all(verbose=False)


# ---- the names and the exception rule -----------------------------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "memvul_claims.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(libs):
    declared = sorted(set(re.findall(r"\b(mvc_[a-z_0-9]+)\s*\(", _header())))
    assert declared == sorted(claims.CLAIMS_SYMBOLS) and len(declared) == 12
    lib = claims.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libmemvul_claims.so does not export {name}"
    exported = subprocess.run([_llvm_tool("llvm-readelf"), "--dyn-syms", build.LIB_PATH_CLAIMS], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mvc_\w+)", exported))) == declared and not re.search(r"\bmvr?_[a-z]", exported)
    macros = dict(re.findall(r"#define (MVC_MAX_\w+) \(?([0-9l< ]+)\)?", open(os.path.join(ROOT, "include", "memvul_claims.h")).read()))
    assert macros["MVC_MAX_THRESHOLDS"].strip() == "64" == str(claims.MAX_THRESHOLDS) and macros["MVC_MAX_VECTORS"].strip() == "4096" == str(claims.MAX_VECTORS)
    assert macros["MVC_MAX_PAIRS"].strip() == "1ll << 28" and claims.MAX_PAIRS == 1 << 28 and int(macros["MVC_MAX_ROWS"].strip("l ")) == claims.MAX_ROWS


def test_no_cpp_exception_can_cross_the_boundary():
    src = open(os.path.join(CSRC, "claims.hip")).read()
    heads = re.findall(r"^int (mvc_\w+)\(([^{;]*?)\)\s*(try\s*)?\{", src, flags=re.M)
    declared = sorted(set(re.findall(r"^\s*int\s+(mvc_\w+)\s*\(", _header(), flags=re.M)))
    assert len(declared) == 9 and sorted(name for name, _, _ in heads) == declared
    assert all(guard for _, _, guard in heads), [name for name, _, guard in heads if not guard]
    assert src.count("catch (...) { return on_exception(") == len(heads)


# ---- the build ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_build_all_still_returns_two_paths_and_leaves_the_new_library_fresh(libs):
    assert list(libs) == [build.LIB_PATH, build.LIB_PATH_DEV]
    assert not build.is_stale() and not build.is_stale(dev=True) and not build.retrieve_is_stale() and not build.tok_is_stale() and not build.claims_is_stale()
    assert os.path.exists(build.LIB_PATH_CLAIMS) and os.path.basename(build.LIB_PATH_CLAIMS) == build.CLAIMS_LIB_NAME == "libmemvul_claims.so"
    assert claims.LIB_PATH == build.LIB_PATH_CLAIMS
    needed = subprocess.run([_llvm_tool("llvm-readelf"), "-d", build.LIB_PATH_CLAIMS], capture_output=True, text=True, check=True).stdout
    assert "libmemvul" not in "".join(ln for ln in needed.splitlines() if "NEEDED" in ln)  # it links against nothing of this tree


def test_the_kernels_are_the_recorded_ones(libs):
    kk.check_kernels_are_the_recorded_ones(build.LIB_PATH_CLAIMS, "claims")


def test_the_other_libraries_do_not_know_the_new_files(libs, monkeypatch):
    new, _ = kk.own_and_shared("claims")
    assert build.SIDE_LIBS["claims"] == (build.CLAIMS_LIB_NAME, build.CLAIMS_SOURCES, build.CLAIMS_HEADERS)
    kk.check_the_shared_headers_belong_to_the_four_kept_libraries(monkeypatch)
    kk.check_the_index_plumbing_is_defined_once()
    assert sorted(os.path.basename(p) for p in new) == ["claim_sweep.h", "claims.hip", "memvul_claims.h"]
    opened = []
    real_open = open

    def spy(path, *a, **kw):
        opened.append(os.path.abspath(path) if isinstance(path, str) else path)
        return real_open(path, *a, **kw)

    monkeypatch.setattr("builtins.open", spy)
    build.source_fingerprint()
    build.source_fingerprint((), build.RETRIEVE_SOURCES, build.RETRIEVE_HEADERS)
    build.source_fingerprint((), build.TOK_SOURCES, build.TOK_HEADERS)
    build.source_fingerprint((), build.BANK_SOURCES, build.BANK_HEADERS)
    monkeypatch.undo()
    assert opened and not set(opened) & set(new)
    for name in os.listdir(CSRC):  # nothing any other library is built from includes the new header
        if name not in ("claims.hip", "claim_sweep.h"):
            assert "claim_sweep.h" not in open(os.path.join(CSRC, name)).read(), name
    src = open(os.path.join(CSRC, "claims.hip")).read() + open(os.path.join(CSRC, "claim_sweep.h")).read()
    assert not re.search(r'#include\s+"(match_topk|report_topk)\.h"', src)
    new_map = build.kernel_fingerprints(build.LIB_PATH_CLAIMS)
    for n in NEW_KERNELS:
        assert any(n in k and k.endswith(".kd") for k in new_map), n
    for other in (build.LIB_PATH, build.LIB_PATH_TOK, build.LIB_PATH_RETRIEVE):
        other_map = build.kernel_fingerprints(other)
        assert other_map and not set(new_map) & set(other_map), other
        assert not [k for k in other_map if any(n in k for n in NEW_KERNELS)], other


def test_no_kernel_uses_scratch_or_spills_and_lds_stays_within_the_cu(libs, tmp_path):
    (co,) = build.device_code_objects(build.LIB_PATH_CLAIMS)
    elf = tmp_path / "gfx950.co"
    elf.write_bytes(co)
    notes = subprocess.run([_llvm_tool("llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True, check=True).stdout
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
    assert len([k for k in kernels if "claim_score_kernel" in k]) == 24  # P 512 / 768 x 64 / 128 / 256 / 512 rows per block x count / mark / fill
    for k, (scratch, lds, spill) in kernels.items():  # (scalar registers parked in lanes of a vector register ahead of the loops are neither)
        assert scratch == 0 and spill == 0 and lds <= 160 * 1024, (k, scratch, lds, spill)


# ---- the plan in numpy ----------------------------------------------------------------------------------------------------------------------------------------------

Q_PLAN = 7


@pytest.fixture(scope="module")
def tie_heavy():
    """P(same) [4099, 7] of the fixture, quantised to 1/32 so that MANY entries equal a threshold exactly, with a NaN row; classes alternate in runs of three."""
    U, V, W = kit.rkit.fixture(11, 4099, 64, Q_PLAN)
    p = (np.round(kit.rkit.psame_f64(U, V, W, 0) * 32) / 32).astype(np.float32)
    p[1234] = np.float32("nan")
    p.setflags(write=False)
    cls = ((np.arange(4099) // 3) % 2).astype(np.uint8)
    return p, cls


TH_PLAN = np.array([0.5, 0.0, 1.0, 1.25, 0.5], np.float32)  # one that equals many entries exactly (twice), 0, 1, above 1


def _ranges(N):
    return [(0, N)] + [(f, c) for f, c in ((1, N - 1), (63, 130), (65, 64), (N - 1, 1), (5, 0)) if f >= 0 and c >= 0 and f + c <= N]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("block_rows", [64, 256])
@pytest.mark.parametrize("vector_group", [1, 5, 7])
def test_the_plan_gives_the_rule(tie_heavy, N, block_rows, vector_group):
    p, cls = tie_heavy[0][:N], tie_heavy[1][:N]
    assert N < 100 or (p == TH_PLAN[0]).sum() > N // 8
    for first, count in _ranges(N) if (block_rows, vector_group) == (64, 5) or N <= 257 else [(0, N), (63, 130)]:
        sub, csub = p[first:first + count], cls[first:first + count]
        want = kit.reference_counts(sub, csub, TH_PLAN)
        got = kit.plan_counts(p, cls, TH_PLAN, first, count, block_rows, vector_group)
        assert got.tobytes() == want.tobytes(), (N, first, count)
        thres = TH_PLAN[np.arange(Q_PLAN) % len(TH_PLAN)]
        want_s = kit.reference_select(sub, thres, first)
        got_s = kit.plan_select(p, thres, first, count, block_rows, vector_group)
        for g, w in zip(got_s, want_s):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (N, first, count)
    if N > 1234:  # the NaN row is never claimed, at threshold 0 either
        off, rows, _ = kit.plan_select(p, np.zeros(Q_PLAN, np.float32), 0, N, block_rows, vector_group)
        assert 1234 not in rows and np.array_equal(np.diff(off), np.full(Q_PLAN, N - 1))


def test_the_rule_by_hand():
    p = np.array([[0.5, 0.1], [0.9, np.nan], [0.5, 0.1], [0.25, 0.3]], np.float32)
    cls = np.array([1, 0, 0, 1], np.uint8)
    c = kit.reference_counts(p, cls, np.array([0.5, 0.0, 0.95], np.float32))
    assert c.tolist() == [[[2, 1], [2, 2], [0, 0]], [[0, 0], [1, 2], [0, 0]]]
    off, rows, ps = kit.reference_select(p, np.array([0.5, 0.1], np.float32), first=10)
    assert off.tolist() == [0, 3, 6] and rows.tolist() == [10, 11, 12, 10, 12, 13] and ps.tolist() == [0.5, np.float32(0.9), 0.5, np.float32(0.1), np.float32(0.1), np.float32(0.3)]
    r2, p2 = kit.by_prob(off, rows, ps)
    assert r2.tolist() == [11, 10, 12, 13, 10, 12]
    r3, p3 = claims.order_by_prob(off, rows, ps)
    assert r3.tolist() == r2.tolist() and p3.tobytes() == p2.tobytes()


@pytest.mark.parametrize("fault", ["gt", "word_base", "dead_lanes", "no_first", "local_class"])
def test_the_plan_model_sees_each_seeded_fault(tie_heavy, fault):
    p, cls = tie_heavy[0][:257], tie_heavy[1][:257]
    first, count = 63, 130  # (ends inside a word: 2 dead lanes... 130 = 2 words + 2 rows)
    thres = TH_PLAN[np.arange(Q_PLAN) % len(TH_PLAN)]
    want_c = kit.reference_counts(p[first:first + count], cls[first:first + count], TH_PLAN)
    want_s = kit.reference_select(p[first:first + count], thres, first)
    seen = False
    if fault in ("gt", "dead_lanes", "local_class"):
        seen = seen or kit.plan_counts(p, cls, TH_PLAN, first, count, 64, 5, fault=fault).tobytes() != want_c.tobytes()
    if fault in ("gt", "dead_lanes", "word_base", "no_first"):
        got = kit.plan_select(p, thres, first, count, 64, 5, fault=fault)
        seen = seen or any(g.tobytes() != w.tobytes() for g, w in zip(got, want_s))
    assert seen, fault
    if fault in ("gt", "dead_lanes"):  # both endings must see these two
        assert kit.plan_counts(p, cls, TH_PLAN, first, count, 64, 5, fault=fault).tobytes() != want_c.tobytes()
        assert any(g.tobytes() != w.tobytes() for g, w in zip(kit.plan_select(p, thres, first, count, 64, 5, fault=fault), want_s))


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_float64_thresholds_are_rounded_up_to_fp32():
    rng = np.random.default_rng(5)
    grid64 = np.arange(0.5, 0.9, 0.01)
    exact = rng.random(2000).astype(np.float32).astype(np.float64)
    near = np.nextafter(exact[:500], 2.0)  # just above an fp32 number: rounds up a whole fp32 step
    t = np.concatenate([grid64, exact, near, rng.random(100000 - len(grid64) - 2500), [0.0, 1.0, -0.25, 1e-300, 5e-324]])
    p = rng.random(len(t)).astype(np.float32)
    p[:3000] = t[:3000].astype(np.float32)  # pairs that sit on, or one step beside, their threshold
    p[3000:6000] = np.nextafter(t[:3000].astype(np.float32), np.float32(-1))
    up = claims.up32(t)
    assert up.dtype == np.float32 and len(t) >= 100000
    assert np.array_equal(p.astype(np.float64) >= t, p >= up)
    assert (up.astype(np.float64) >= t).all() and (np.nextafter(up, np.float32(-np.inf)).astype(np.float64) < t).all()  # the SMALLEST fp32 at or above t
    assert claims.up32(exact).tobytes() == exact.astype(np.float32).tobytes()
    assert claims.up32(0.51) > np.float32(0.51) or np.float64(np.float32(0.51)) >= 0.51
    for bad in (np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError):
            claims.up32(bad)


def test_the_reference_grid():
    g = claims.reference_grid()
    want64 = np.arange(0.5, 0.9, 0.01)
    assert g.dtype == np.float32 and g.shape == (40,) and len(want64) == 40
    for x, t in zip(g.tolist(), want64.tolist()):  # rounded up, checked in exact arithmetic
        assert Fraction(x) >= Fraction(t) and Fraction(float(np.nextafter(np.float32(x), np.float32(-1)))) < Fraction(t)
    assert g[0] == 0.5 and g[1] != np.float32(0.51) and float(g[1]) > 0.51  # 0.51 is not an fp32 number, and the nearest one lies below it
    assert claims.parse_grid("reference").tobytes() == want64.tobytes() and claims.parse_grid("0.1:0.35:0.1").tolist() == np.arange(0.1, 0.35, 0.1).tolist()
    for bad in ("0.5:0.4:0.1", "0.5:0.9", "0.5:0.9:0", "0:1:0.001"):
        with pytest.raises(ValueError):
            claims.parse_grid(bad)


# ---- validation before any library call --------------------------------------------------------------------------------------------------------------------------------

class _StubLib(kk.StubLib):
    PREFIX = "mvc_"

    def counts(self, h, v, Q, th, T, first, count, out):
        self._thresholds(th, T)
        self.log.append(("counts", Q, T, first, count))
        return 0

    def select(self, h, v, Q, th, first, count, off):
        self._thresholds(th, Q)
        self.log.append(("select", Q, first, count))
        o = C.cast(off, C.POINTER(C.c_int64))
        for i in range(Q + 1):
            o[i] = 0
        return 0

    def fetch(self, h, r, p):
        self.log.append(("fetch",))
        return 0


W512 = kk.W512


def test_bad_arguments_raise_before_any_call():
    lib = _StubLib()
    for args in ((0, 500, W512, 0), (0, 512, W512, 2), (0, 512, W512[:, :100], 0), (0, 512, W512.astype(np.float64), 0), (-1, 512, W512, 0), (0, 512.0, W512, 0)):
        with pytest.raises((ValueError, TypeError)):
            claims.ClaimIndex(*args, lib=lib)
    assert lib.log == []
    with claims.ClaimIndex(0, 512, W512, 1, lib=lib) as ix:
        assert lib.log == [("create", 0, 512, 1)]
        ok = np.zeros((10, 512), np.float32)
        for bad in (ok.astype(np.float64), ok[:, :500], ok[:, ::2], np.zeros((10, 1024), np.float32)[:, ::2], ok.tolist(), ok[0]):
            with pytest.raises((ValueError, TypeError)):
                ix.add(bad)
        assert len(lib.log) == 1
        ix.add(ok)
        assert lib.log[-1] == ("add", 10) and len(ix) == 10
        n_calls = len(lib.log)
        v = np.zeros((3, 512), np.float32)
        th = [0.5, 0.6]
        calls = (lambda: ix.counts(v, []), lambda: ix.counts(v, [0.5] * 65), lambda: ix.counts(v, 0.5), lambda: ix.counts(v, [0.5, np.nan]), lambda: ix.counts(v, [np.inf]),
                 lambda: ix.counts(v, np.array([1, 2])), lambda: ix.counts(v, np.array([[0.5]])), lambda: ix.counts(v, ["0.5"]), lambda: ix.counts(v, th, -1),
                 lambda: ix.counts(v, th, 5, 6), lambda: ix.counts(v, th, 11), lambda: ix.counts(v, th, 0, -1), lambda: ix.counts(v, th, 0.0), lambda: ix.counts(v[:0], th),
                 lambda: ix.counts(np.zeros((4097, 512), np.float32), th), lambda: ix.counts(v.astype(np.float16), th), lambda: ix.counts(np.zeros((3, 768), np.float32), th),
                 lambda: ix.counts(np.asfortranarray(v), th), lambda: ix.counts(v.tolist(), th),
                 lambda: ix.select(v, [0.5, 0.6]), lambda: ix.select(v, np.nan), lambda: ix.select(v, "0.5"), lambda: ix.select(v, True), lambda: ix.select(v, 0.5, order="rank"),
                 lambda: ix.select(v, 0.5, 3, 8), lambda: ix.select(v[:0], 0.5), lambda: ix.select(v.astype(np.float64), 0.5), lambda: ix.select(v, np.zeros(3, np.float16)),
                 lambda: ix.set_classes(np.zeros(11, np.uint8)), lambda: ix.set_classes(np.zeros(5, np.uint8), 6), lambda: ix.set_classes(np.full(3, 2, np.uint8)),
                 lambda: ix.set_classes(np.zeros(3, np.int64)), lambda: ix.set_classes([0, 1]), lambda: ix.set_classes(np.zeros((2, 2), np.uint8)),
                 lambda: ix.set_classes(np.zeros(3, np.uint8), -1))
        for i, call in enumerate(calls):
            with pytest.raises((ValueError, TypeError)):
                call()
            assert len(lib.log) == n_calls, i
        with pytest.raises(ValueError, match="2\\^31"):
            lib.n = 2 ** 31 - 5
            ix.add(ok)
        lib.n = 10
        assert len(lib.log) == n_calls
        # what reaches the library: fp32, float64 rounded UP, fp32 taken as it is
        c = ix.counts(v, [0.51, 0.5], 2)
        assert lib.log[-1] == ("counts", 3, 2, 2, 8) and c.shape == (3, 2, 2) and c.dtype == np.int64
        assert lib.th.tolist() == [float(np.nextafter(np.float32(0.51), np.float32(1))), 0.5] and float(lib.th[0]) > 0.51
        ix.counts(v, np.array([0.51], np.float32))
        assert lib.th.tolist() == [float(np.float32(0.51))]
        ix.counts(v, claims.reference_grid())
        assert lib.log[-1] == ("counts", 3, 40, 0, 10) and lib.th.tobytes() == claims.reference_grid().tobytes()
        off, rows, p = ix.select(v, 0.51, 1, 3)
        assert lib.log[-2:] == [("select", 3, 1, 3), ("fetch",)] and lib.th.tolist() == [float(np.nextafter(np.float32(0.51), np.float32(1)))] * 3
        assert off.tolist() == [0, 0, 0, 0] and rows.dtype == np.int64 and p.dtype == np.float32 and len(rows) == len(p) == 0
        ix.select(v, np.float32(0.51))  # an fp32 number is its own threshold
        assert lib.th.tolist() == [float(np.float32(0.51))] * 3
        ix.select(v, np.float64(0.51))
        assert lib.th.tolist() == [float(np.nextafter(np.float32(0.51), np.float32(1)))] * 3
        ix.select(v, np.array([0.1, 0.2, 0.3])[::-1], order="row")
        assert lib.th.tobytes() == claims.up32([0.3, 0.2, 0.1]).tobytes()
        ix.select(v, np.array([0.1, 0.2, 0.3]), order="row")
        assert lib.th.tobytes() == claims.up32([0.1, 0.2, 0.3]).tobytes()
        ix.set_classes(np.array([True, False, True]), 7)
        assert lib.log[-1] == ("classes", 7, 3)
        ix.test_plan(64, 5)
        assert lib.log[-1] == ("plan", 64, 5)
        with pytest.raises(RuntimeError, match="stub"):
            ix.kernel_ms()
        ix.reset()
        assert len(ix) == 0
    assert lib.log[-1] == ("destroy",)
    with pytest.raises(RuntimeError, match="closed"):
        ix.counts(v, th)


# ---- ModelMemory.anchor_claims and the command line on the stand-in -----------------------------------------------------------------------------------------------------

def _want_entries(ps, same, thres, urls, first=0):
    out = []
    for g in range(ps.shape[1]):
        r = [int(i) for i in np.flatnonzero(ps[:, g].astype(np.float64) >= thres[g])]  # the reference's comparison: float(p32) >= t
        r.sort(key=lambda i: (-float(ps[i, g]), i))
        out.append(dict(claimed=len(r), positives=int(same[r].sum()), rows=[first + i for i in r], urls=[urls[first + i] for i in r]))
    return out


def test_anchor_claims_on_the_standin(standin_model):
    model, arrays, fx = standin_model
    _, _, ps = model.sweep_arrays(arrays, batch_size=8, with_probs=True, keep=True)
    ps = ps.astype(np.float32)
    same = np.asarray(arrays["same"], bool)
    thres = float(np.median(ps))  # about half of the pairs
    out = model.anchor_claims(arrays, thres, index_factory=_NumpyClaims)
    assert [e["anchor"] for e in out] == model._golden_labels == [f"CWE-{100 + i}" for i in range(4)]
    want = _want_entries(ps, same, [thres] * 4, arrays["urls"])
    assert 0 < sum(w["claimed"] for w in want) < ps.size
    for e, w in zip(out, want):
        assert set(e) == {"anchor", "thres", "claimed", "positives", "reports"} and e["thres"] == thres
        assert (e["claimed"], e["positives"]) == (w["claimed"], w["positives"])
        assert [r["row"] for r in e["reports"]] == w["rows"] and [r["Issue_Url"] for r in e["reports"]] == w["urls"]
        assert all(set(r) == {"Issue_Url", "row", "prob"} and r["prob"] >= thres for r in e["reports"])
    json.dumps(out)
    ix = _NumpyClaims.made[0]
    assert len(_NumpyClaims.made) == 1 and np.array_equal(ix.w, fx[4]["_projector.weight"]) and ix.u.shape == (23, 512) and np.array_equal(ix.cls, same.astype(np.uint8))
    # the claim index and the report index from one download; the host copy is let go once those two are filled
    assert _CountingEngine.downloads == 1 and model._kept.embed is not None
    model.anchor_reports(arrays, 5, index_factory=_NumpyIndex)
    assert _CountingEngine.downloads == 1 and len(_NumpyIndex.made) == 1 and _NumpyIndex.made[0].u.shape == (23, 512) and model._kept.embed is None
    # one threshold per vector, given vectors and labels, a grid
    v = model.engine.anchor_get()[[2, 0]]
    th2 = [float(np.percentile(ps[:, 2], 80)), float(np.percentile(ps[:, 0], 20))]
    grid = [0.2, 0.5, float(np.median(ps)), 0.8]
    out2 = model.anchor_claims(arrays, th2, vectors=v, labels=["fresh CVE", "another"], grid=grid, index_factory=_NumpyClaims)
    assert len(_NumpyClaims.made) == 1 and _CountingEngine.downloads == 1
    want2 = _want_entries(ps[:, [2, 0]], same, th2, arrays["urls"])
    for e, w, t in zip(out2, want2, th2):
        assert e["thres"] == t and e["claimed"] == w["claimed"] and [r["row"] for r in e["reports"]] == w["rows"]
    assert [e["anchor"] for e in out2] == ["fresh CVE", "another"]
    for g, e in zip((2, 0), out2):
        assert [x["thres"] for x in e["grid"]] == grid
        for x in e["grid"]:
            claimed = ps[:, g].astype(np.float64) >= x["thres"]
            assert (x["claimed"], x["positives"]) == (int(claimed.sum()), int((claimed & same).sum()))
        assert e["best_thres"] in grid
    assert [e["anchor"] for e in model.anchor_claims(arrays, 0.5, vectors=v, index_factory=_NumpyClaims)] == ["0", "1"]
    assert len(model.anchor_claims(arrays, grid="reference", index_factory=_NumpyClaims)[0]["grid"]) == 40
    for bad in (dict(vectors=v, thres=[0.5, 0.5, 0.5]), dict(grid="nonsense"), dict(grid=[0.5] * 65), dict(thres=float("nan"))):
        with pytest.raises(ValueError):
            model.anchor_claims(arrays, index_factory=_NumpyClaims, **bad)
    # a new sweep drops every index: of rows 4 .. 20 now, numbered as in `arrays`, classes of those rows
    first_index = _NumpyClaims.made[0]
    _, _, ps = model.sweep_arrays(arrays, 4, 20, batch_size=8, with_probs=True, keep=True)
    ps = ps.astype(np.float32)
    assert first_index.closed and _NumpyIndex.made[0].closed and model._kept.embed is None
    out3 = model.anchor_claims(arrays, thres, 4, 20, index_factory=_NumpyClaims)
    assert len(_NumpyClaims.made) == 2 and _NumpyClaims.made[1].u.shape == (16, 512) and np.array_equal(_NumpyClaims.made[1].cls, same[4:20].astype(np.uint8))
    want3 = _want_entries(ps, same[4:20], [thres] * 4, arrays["urls"], first=4)
    for e, w in zip(out3, want3):
        assert [r["row"] for r in e["reports"]] == w["rows"] and [r["Issue_Url"] for r in e["reports"]] == w["urls"] and e["positives"] == w["positives"]
    assert _CountingEngine.downloads == 2


def test_best_thres_by_hand():
    """Six rows, three of them positive.  At 0.5 all six are claimed (F1 2/3); at 0.65 and at 0.68 exactly the three positives (F1 1, a tie: the LAST wins, as the
    reference's `>=` has it); at 0.85 one (F1 1/2)."""
    p = np.array([0.9, 0.7, 0.8, 0.6, 0.55, 0.52], np.float32)[:, None]
    cls = np.array([1, 1, 1, 0, 0, 0], np.uint8)
    grid = [0.5, 0.65, 0.68, 0.85]
    counts = kit.reference_counts(p, cls, claims.up32(grid))
    assert counts[0].tolist() == [[3, 3], [0, 3], [0, 3], [0, 1]]
    t, m = claims.best_threshold(grid, counts[0], 3, 3)
    assert t == 0.68 and m["f1"] == 1 and (m["TP"], m["FN"], m["TN"], m["FP"]) == (3, 0, 3, 0)
    assert claims.best_threshold(grid[::-1], counts[0][::-1], 3, 3)[0] == 0.65  # visited the other way round, the other end of the tie
    # nothing positive anywhere: every F1 is 0 and `>=` walks to the last threshold
    assert claims.best_threshold(grid, np.zeros((4, 2), np.int64), 0, 6)[0] == 0.85
    # the same through the entries, and against find_best_thres itself on the column
    from memvul_amd.custom_metric import find_best_thres

    class _Index:
        def counts(self, v, thresholds, first=0, count=None):
            return kit.reference_counts(p, cls, claims.up32(thresholds))

        def select(self, v, thres, first=0, count=None, order="prob"):
            off, rows, pp = kit.reference_select(p, claims.up32(thres))
            return (off,) + tuple(kit.by_prob(off, rows, pp))

    (e,) = claims.claims_of(_Index(), ["a"], [f"u{i}" for i in range(6)], np.zeros((1, 512), np.float32), 0.6, cls.astype(bool), 0, grid)
    assert e["best_thres"] == 0.68 and (e["claimed"], e["positives"]) == (4, 3) and [r["row"] for r in e["reports"]] == [0, 2, 1, 3]
    assert [(x["claimed"], x["positives"]) for x in e["grid"]] == [(6, 3), (3, 3), (3, 3), (1, 1)]
    (e,) = claims.claims_of(_Index(), ["a"], [f"u{i}" for i in range(6)], np.zeros((1, 512), np.float32), 0.6, cls.astype(bool), 0, "reference", with_reports=False)
    assert "reports" not in e and (e["claimed"], e["positives"]) == (4, 3)
    assert e["best_thres"] == find_best_thres(cls, p[:, 0])["thres"]


def test_the_command_line_writes_one_json_line_per_anchor(capsys, tmp_path):
    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=12, n_anchors=4, layers=2)
    try:
        _KeepingEngine.created, _NumpyClaims.made = [], []
        out = tmp_path / "claims.jsonl"
        std = ["--archive", arch, "--golden", golden, "--input", test_path]
        eng0 = _KeepingEngine  # the first run tells what P(same) is; the threshold is taken from it
        rc = claims.main(std + ["--thres", "0.0", "--out", str(out)], engine_factory=eng0, index_factory=_NumpyClaims)
        lines = [json.loads(ln) for ln in open(out)]
        assert rc == 0 and [e["anchor"] for e in lines] == [f"CWE-{100 + i}" for i in range(4)] and all(e["claimed"] == 12 == len(e["reports"]) for e in lines)
        assert capsys.readouterr().out.strip() == "" and _NumpyClaims.made[0].closed
        eng = _KeepingEngine.created[0]
        ids, lens, arrs = _inputs(arch, golden, test_path)
        ps = eng.forward(ids, lens)["probs"][:, :, 0].astype(np.float32)
        urls, same = arrs["urls"], np.asarray(arrs["same"], bool)
        assert np.array_equal(_NumpyClaims.made[0].cls, same.astype(np.uint8))
        thres = float(np.median(ps))
        rc = claims.main(std + ["--thres", repr(thres), "--grid", "0.2:0.85:0.05", "--anchors", "CWE-102,CWE-100"], engine_factory=eng0, index_factory=_NumpyClaims)
        printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        want = _want_entries(ps[:, [2, 0]], same, [thres, thres], urls)
        assert rc == 0 and [e["anchor"] for e in printed] == ["CWE-102", "CWE-100"]
        for e, x in zip(printed, want):
            assert [r["row"] for r in e["reports"]] == x["rows"] and [r["Issue_Url"] for r in e["reports"]] == x["urls"] and e["positives"] == x["positives"]
            assert [g["thres"] for g in e["grid"]] == np.arange(0.2, 0.85, 0.05).tolist() and e["best_thres"] in [g["thres"] for g in e["grid"]]
        rc = claims.main(std + ["--thres", repr(thres), "--counts-only", "--grid", "reference"], engine_factory=eng0, index_factory=_NumpyClaims)
        printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        want = _want_entries(ps, same, [thres] * 4, urls)
        assert rc == 0 and all("reports" not in e and len(e["grid"]) == 40 for e in printed)
        assert [(e["claimed"], e["positives"]) for e in printed] == [(x["claimed"], x["positives"]) for x in want]
        for bad in (["--anchors", "CWE-999"], ["--grid", "1:0:0.1"], ["--thres", "nan"]):
            with pytest.raises(SystemExit):
                claims.main(std + bad, engine_factory=eng0, index_factory=_NumpyClaims)
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- no GPU, no index -------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_constructor_raises_without_a_gpu(libs):
    try:
        has_gpu = subprocess.run(["/opt/rocm/bin/rocm_agent_enumerator"], capture_output=True, text=True).stdout.count("gfx9") > 0
    except Exception:
        has_gpu = False
    with pytest.raises(RuntimeError, match="mvc_create"):
        claims.ClaimIndex(4096 if has_gpu else 0, 512, W512, 0)  # (with a GPU: a device that is not there)
    with pytest.raises(RuntimeError, match="not found"):
        claims.load_library(os.path.join(ROOT, "memvul_amd", "lib", "no_such_library.so"))
    assert not hasattr(binding, "CLAIMS_SYMBOLS") and not set(claims.CLAIMS_SYMBOLS) & set(retrieve.RETRIEVE_SYMBOLS)
