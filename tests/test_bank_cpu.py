"""The anchor-bank audit (memvul_amd/bank.py, libmemvul_bank.so): what needs no GPU — the names, the build, the built kernels' resources, the plan in numpy against
the definitions it must reproduce (and the faults it must see), the audit document by hand, the Python validation on a recording stub, and
ModelMemory.anchor_bank_audit / the command line on the oracle-backed stand-in."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from memvul_amd import bank, binding, build, claims, retrieve

import bank_kit as kit
import kept_index_kit as kk
import plumbing_util as pu
from kept_index_kit import _CountingEngine, _KeepingEngine, _NumpyBank, _NumpyClaims, _NumpyIndex, _inputs, standin_model  # noqa: F401  (standin_model is a fixture)
from test_f32_form_cpu import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memvul_amd", "csrc")
NEW_KERNELS = ("bank_weight_delta_kernel", "bank_row_term_kernel", "bank_vector_prep_kernel", "bank_mark_kernel", "bank_class_words_kernel", "bank_totals_kernel",
               "bank_multiplicity_kernel", "bank_overlap_kernel", "bank_mirror_kernel", "bank_cover_init_kernel", "bank_gain_kernel", "bank_pick_kernel")


@pytest.fixture(scope="module")
def libs():
    return build.build_all(verbose=False)


# ---- the names and the exception rule -----------------------------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "memvul_bank.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(libs):
    declared = sorted(set(re.findall(r"\b(mvb_[a-z_0-9]+)\s*\(", _header())))
    assert declared == sorted(bank.BANK_SYMBOLS) and len(declared) == 14
    lib = bank.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libmemvul_bank.so does not export {name}"
    exported = subprocess.run([_llvm_tool("llvm-readelf"), "--dyn-syms", build.LIB_PATH_BANK], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mvb_\w+)", exported))) == declared
    assert not re.search(r"\bmv[rc]?_[a-z]", exported)  # no mv_, mvr_ or mvc_ name
    raw = open(os.path.join(ROOT, "include", "memvul_bank.h")).read()
    macros = dict(re.findall(r"#define (MVB_MAX_\w+) \(?([0-9l< ]+)\)?", raw))
    assert macros["MVB_MAX_VECTORS"].strip() == "4096" == str(bank.MAX_VECTORS) and int(macros["MVB_MAX_ROWS"].strip("l ")) == bank.MAX_ROWS
    assert macros["MVB_MAX_WEIGHT"].strip() == "1 << 20" and bank.MAX_WEIGHT == 1 << 20
    assert macros["MVB_MAX_MARK_BYTES"].strip() == "4ll << 30" and bank.MAX_MARK_BYTES == 4 << 30
    assert not set(bank.BANK_SYMBOLS) & (set(claims.CLAIMS_SYMBOLS) | set(retrieve.RETRIEVE_SYMBOLS)) and not hasattr(binding, "BANK_SYMBOLS")


def test_no_cpp_exception_can_cross_the_boundary():
    src = open(os.path.join(CSRC, "bank.hip")).read()
    heads = re.findall(r"^int (mvb_\w+)\(([^{;]*?)\)\s*(try\s*)?\{", src, flags=re.M)
    declared = sorted(set(re.findall(r"^\s*int\s+(mvb_\w+)\s*\(", _header(), flags=re.M)))
    assert len(declared) == 11 and sorted(name for name, _, _ in heads) == declared
    assert all(guard for _, _, guard in heads), [name for name, _, guard in heads if not guard]
    assert src.count("catch (...) { return on_exception(") == len(heads)


# ---- the build ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_build_all_leaves_five_fresh_libraries_and_returns_two_paths(libs):
    assert list(libs) == [build.LIB_PATH, build.LIB_PATH_DEV]
    assert not build.is_stale() and not build.is_stale(dev=True) and not build.tok_is_stale() and not build.retrieve_is_stale() and not build.claims_is_stale()
    assert not build.bank_is_stale()
    assert os.path.exists(build.LIB_PATH_BANK) and os.path.basename(build.LIB_PATH_BANK) == build.BANK_LIB_NAME == "libmemvul_bank.so"
    assert bank.LIB_PATH == build.LIB_PATH_BANK and build.build_bank(verbose=False) == build.LIB_PATH_BANK
    needed = subprocess.run([_llvm_tool("llvm-readelf"), "-d", build.LIB_PATH_BANK], capture_output=True, text=True, check=True).stdout
    assert "libmemvul" not in "".join(ln for ln in needed.splitlines() if "NEEDED" in ln)  # it links against nothing of this tree
    for other in (build.LIB_PATH, build.LIB_PATH_DEV, build.LIB_PATH_TOK, build.LIB_PATH_RETRIEVE, build.LIB_PATH_CLAIMS):  # and nothing links against it
        needed = subprocess.run([_llvm_tool("llvm-readelf"), "-d", other], capture_output=True, text=True, check=True).stdout
        assert "libmemvul_bank" not in needed, other


def test_the_kernels_are_the_recorded_ones(libs):
    kk.check_kernels_are_the_recorded_ones(build.LIB_PATH_BANK, "bank")


def test_the_module_prints_the_new_path_too():
    src = open(os.path.join(ROOT, "memvul_amd", "build.py")).read()
    assert re.search(r'__name__ == "__main__":\n\s+print\(.*LIB_PATH_BANK', src)


def test_the_other_libraries_do_not_know_the_new_files(libs, monkeypatch):
    new, _ = kk.own_and_shared("bank")
    assert build.SIDE_LIBS["bank"] == (build.BANK_LIB_NAME, build.BANK_SOURCES, build.BANK_HEADERS)
    kk.check_the_shared_headers_belong_to_the_four_kept_libraries(monkeypatch)
    assert sorted(os.path.basename(p) for p in new) == ["bank.hip", "bank_cover.h", "memvul_bank.h"]
    opened = []
    real_open = open

    def spy(path, *a, **kw):
        opened.append(os.path.abspath(path) if isinstance(path, str) else path)
        return real_open(path, *a, **kw)

    monkeypatch.setattr("builtins.open", spy)
    build.source_fingerprint()
    build.source_fingerprint((), build.RETRIEVE_SOURCES, build.RETRIEVE_HEADERS)
    build.source_fingerprint((), build.CLAIMS_SOURCES, build.CLAIMS_HEADERS)
    build.source_fingerprint((), build.TOK_SOURCES, build.TOK_HEADERS)
    monkeypatch.undo()
    assert opened and not set(opened) & set(new)
    for name in os.listdir(CSRC):  # nothing any other library is built from includes the new header, and the new files include none of theirs
        text = open(os.path.join(CSRC, name)).read()
        if name not in ("bank.hip", "bank_cover.h"):
            assert "bank_cover.h" not in text and "memvul_bank.h" not in text, name
    src = open(os.path.join(CSRC, "bank.hip")).read() + open(os.path.join(CSRC, "bank_cover.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["../../include/memvul_bank.h", "bank_cover.h", "kept_index.h", "kept_terms.h"]
    new_map = build.kernel_fingerprints(build.LIB_PATH_BANK)
    for n in NEW_KERNELS:
        assert any(n in k and k.endswith(".kd") for k in new_map), n
    for other in (build.LIB_PATH, build.LIB_PATH_TOK, build.LIB_PATH_RETRIEVE, build.LIB_PATH_CLAIMS):
        other_map = build.kernel_fingerprints(other)
        assert other_map and not set(new_map) & set(other_map), other
        assert not [k for k in other_map if any(n in k for n in NEW_KERNELS)], other


def test_no_kernel_uses_scratch_or_spills_and_lds_stays_within_the_cu(libs, tmp_path):
    (co,) = build.device_code_objects(build.LIB_PATH_BANK)
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
    assert len([k for k in kernels if "bank_mark_kernel" in k]) == 8  # P 512 / 768 x 64 / 128 / 256 / 512 rows per block
    assert len(kernels) == 21
    for k, (scratch, lds, spill) in kernels.items():
        assert scratch == 0 and spill == 0 and lds <= 160 * 1024, (k, scratch, lds, spill)


def test_the_marking_size_rule():
    """MVB_MAX_MARK_BYTES on the Python restatement (the library refuses by the same arithmetic before it allocates; a small index cannot reach it)."""
    assert bank.mark_bytes(1, 1) == 8 == kit.mark_bytes(1, 1) and bank.mark_bytes(37, 4099) == 8 * 37 * 65 and bank.mark_bytes(5, 0) == 0
    for Q, count in ((1, 64), (124, 1_200_000), (1000, 1_200_000), (4096, 2 ** 31 - 2), (4096, 8_388_608), (4096, 8_388_609), (16, 2 ** 31 - 2)):
        assert bank.mark_bytes(Q, count) == kit.mark_bytes(Q, count)
    assert bank.mark_bytes(4096, 8_388_608) == bank.MAX_MARK_BYTES and bank.mark_bytes(4096, 8_388_609) > bank.MAX_MARK_BYTES
    assert bank.mark_bytes(1000, 1_200_000) == 150_000_000  # the issue's size: 1.2 M reports, 1 000 vectors
    assert bank.mark_bytes(16, 2 ** 31 - 2) <= bank.MAX_MARK_BYTES < bank.mark_bytes(17, 2 ** 31 - 2)
    lib = _StubLib()
    with bank.BankAudit(0, 512, W512, 0, lib=lib) as ix:
        lib.n = 2 ** 31 - 2
        with pytest.raises(ValueError, match="at most 4294967296"):
            ix.mark(np.zeros((17, 512), np.float32), 0.5)
        assert [c[0] for c in lib.log] == ["create"]


def test_up32_is_the_claims_rule():
    assert bank.up32 is claims.up32 and bank._thresholds is claims._thresholds


# ---- the plan in numpy ----------------------------------------------------------------------------------------------------------------------------------------------

Q_PLAN = 7
TH_PLAN = np.array([0.5, 0.625, 0.75, 0.625, 1.25, 0.375, 0.5], np.float32)  # the duplicate vectors (0 / 6, 1 / 3) share a threshold; one above 1 claims nothing


@pytest.fixture(scope="module")
def tie_heavy():
    """P(same) [4099, 7] of the fixture, quantised to 1/32 so that MANY entries equal a threshold exactly, with a NaN row; classes alternate in runs of three."""
    U, V, W = kit.rkit.fixture(11, 4099, 64, Q_PLAN)
    p = (np.round(kit.rkit.psame_f64(U, V, W, 0) * 32) / 32).astype(np.float32)
    p[1234] = np.float32("nan")
    p.setflags(write=False)
    cls = ((np.arange(4099) // 3) % 2).astype(np.uint8)
    return p, cls


def _ranges(N):
    return [(0, N)] + [(f, c) for f, c in ((1, N - 1), (63, 130), (65, 64), (N - 1, 1), (5, 0)) if f >= 0 and c >= 0 and f + c <= N]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1300])
@pytest.mark.parametrize("plan", [(64, 1, 1), (64, 5, 3), (256, 7, 16), (512, 3, 1000)])
def test_the_plan_gives_the_definitions(tie_heavy, N, plan):
    p, cls = tie_heavy[0][:N], tie_heavy[1][:N]
    assert N < 100 or (p == TH_PLAN[0]).sum() > N // 8
    for first, count in _ranges(N) if plan == (64, 5, 3) or N <= 257 else [(0, N), (63, 130)]:
        for weights in ((1, 1), (2, 1)):
            want = kit.definition_audit(p, cls, TH_PLAN, first, count, *weights)
            got = kit.plan_audit(p, cls, TH_PLAN, first, count, *plan, *weights)
            assert kit.same(got, want) == [], (N, first, count, weights)
            assert np.array_equal(want["overlap"][np.arange(Q_PLAN), np.arange(Q_PLAN)], want["totals"]) and np.array_equal(want["overlap"], want["overlap"].transpose(1, 0, 2))
    if N > 1234:  # the NaN row is never claimed, at threshold 0 either
        got = kit.plan_audit(p, cls, np.zeros(Q_PLAN, np.float32), 0, N, *plan)
        assert got["mult"][1234] == 0 and (np.delete(got["mult"], 1234) == Q_PLAN).all() and got["hist"][:, 0].sum() == 1


def test_the_greedy_cover_by_hand_and_its_stop_rules(tie_heavy):
    p, cls = tie_heavy[0][:1300], tie_heavy[1][:1300]
    want = kit.definition_audit(p, cls, TH_PLAN, 0, 1300, 2, 1)
    assert len(want["order"]) >= 2 and want["tied"] >= 1, (want["order"], want["tied"])  # a round is won by one of two equal vectors: the lower index
    dup = {0: 6, 1: 3}
    assert any(int(q) in dup for q in want["order"]) and not any(int(q) in dup.values() for q in want["order"])
    for look in (1, 2, 8):  # how often the host looks changes nothing
        got = kit.plan_audit(p, cls, TH_PLAN, 0, 1300, 64, 5, 3, 2, 1, look_every=look)
        assert kit.same(got, want) == []
    for kw in (dict(max_rounds=1), dict(max_rounds=0), dict(fixed=np.array([0, 1, 0, 0, 0, 0, 0], np.uint8)), dict(fixed=np.ones(Q_PLAN, np.uint8))):
        w2 = kit.definition_audit(p, cls, TH_PLAN, 0, 1300, 2, 1, **kw)
        assert kit.same(kit.plan_audit(p, cls, TH_PLAN, 0, 1300, 64, 5, 3, 2, 1, **kw), w2) == [], kw
        assert len(w2["order"]) <= kw.get("max_rounds", Q_PLAN) and not (set(w2["order"].tolist()) & set(np.flatnonzero(kw.get("fixed", np.zeros(Q_PLAN))).tolist()))
    assert len(kit.definition_audit(p, cls, TH_PLAN, 0, 1300, 0, 1)["order"]) == 0  # w_pos = 0: no gain is positive
    # three rows, two vectors, by hand: q0 claims rows 0, 1 (pos, neg), q1 claims rows 1, 2 (neg, pos)
    B = np.array([[1, 0], [1, 1], [0, 1]], bool)
    c = np.array([1, 0, 1], np.uint8)
    o, g, tied = kit.greedy(B, c, 2, 1)
    assert o.tolist() == [0, 1] and g.tolist() == [[1, 1], [1, 0]] and tied == 1
    o, g, tied = kit.greedy(B, c, 1, 1)
    assert o.tolist() == [] and tied == 0  # both gains are 0


@pytest.mark.parametrize("fault", kit.FAULTS)
def test_the_plan_model_sees_each_seeded_fault(tie_heavy, fault):
    p, cls = tie_heavy[0][:257], tie_heavy[1][:257]
    first, count = 63, 130  # (ends inside a word)
    fixed = None
    want = kit.definition_audit(p, cls, TH_PLAN, first, count, 2, 1)
    if fault == "fixed_picked":  # the first pick of the free run is fixed: a plan that loses the mask picks it
        fixed = np.zeros(Q_PLAN, np.uint8)
        fixed[want["order"][0]] = 1
        want = kit.definition_audit(p, cls, TH_PLAN, first, count, 2, 1, fixed)
    if fault == "tie_high":
        assert want["tied"] >= 1
    assert kit.same(kit.plan_audit(p, cls, TH_PLAN, first, count, 64, 5, 2, 2, 1, fixed), want) == []
    got = kit.plan_audit(p, cls, TH_PLAN, first, count, 64, 5, 2, 2, 1, fixed, fault=fault)
    seen = kit.same(got, want)
    assert seen, fault
    must = {"gt": {"bits", "totals", "mult"}, "dead_lanes": {"bits", "totals"}, "local_class": {"totals", "hist"}, "tie_high": {"order"}, "fixed_picked": {"order"},
            "diag_twice": {"overlap"}}[fault]
    assert must <= set(seen), (fault, seen)


# ---- the audit document ---------------------------------------------------------------------------------------------------------------------------------------------

def test_audit_of_by_hand():
    """Six rows, three anchors.  Rows 0 .. 2 are positive.  a claims 0, 1, 3; b claims 1, 2; c claims 3 only.  Row 4, 5 unclaimed (negatives), every positive claimed."""
    B = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 1], [0, 0, 0], [0, 0, 0]], bool)
    cls = np.array([1, 1, 1, 0, 0, 0], np.uint8)
    hist, sole, mult, sole_of = kit.multiplicity(B, cls)
    assert hist.tolist() == [[2, 0, 1, 0], [0, 2, 1, 0]] and sole.tolist() == [[0, 1], [0, 1], [0, 0]]
    assert mult.tolist() == [1, 2, 1, 2, 0, 0] and sole_of.tolist() == [0, -1, 1, -1, -1, -1]
    tot, ov = kit.totals(B, cls), kit.overlap(B, cls)
    assert tot.tolist() == [[1, 2], [0, 2], [1, 0]] and ov[0, 1].tolist() == [0, 1] and ov[0, 2].tolist() == [1, 0] and ov[1, 2].tolist() == [0, 0]
    order, gained, _ = kit.greedy(B, cls, 1, 1)
    assert order.tolist() == [1] and gained.tolist() == [[2, 0]]  # b first (gain 2); then a would add row 0 and row 3: gain 0 -> stop
    doc = bank.audit_of(["a", "b", "c"], [0.5, 0.6, 0.7], 3, 3, tot, hist, sole, ov, order, gained, top=2)
    assert doc["union"] == dict(TP=3, FP=1, FN=0, TN=2, precision=0.75, recall=1.0, f1=2 * 0.75 / 1.75)
    assert [a["anchor"] for a in doc["anchors"]] == ["a", "b", "c"] and [a["thres"] for a in doc["anchors"]] == [0.5, 0.6, 0.7]
    assert [a["claimed"] for a in doc["anchors"]] == [[1, 2], [0, 2], [1, 0]] and [a["sole"] for a in doc["anchors"]] == [[0, 1], [0, 1], [0, 0]]
    # without a: TP 2, FP 1, FN 1 -> precision 2/3, recall 2/3; without c nothing changes
    assert doc["anchors"][0]["f1_without"] == pytest.approx(2 / 3) and doc["anchors"][2]["f1_without"] == doc["union"]["f1"]
    # Jaccard: a-c 1/3, a-b 1/4, b-c 0/3
    assert [(o["a"], o["b"], o["both"]) for o in doc["overlaps"]] == [("a", "c", [1, 0]), ("a", "b", [0, 1])]
    assert doc["overlaps"][0]["jaccard"] == pytest.approx(1 / 3) and doc["overlaps"][1]["jaccard"] == 0.25
    assert doc["greedy"] == [dict(anchor="b", index=1, new_pos=2, new_neg=0, TP=2, FP=0)]
    assert doc["rows"] == 6 and doc["positives"] == 3
    json.dumps(doc)
    with pytest.raises(ValueError):
        bank.audit_of(["a", "b", "c"], 0.5, 4, 2, tot, hist, sole, ov)
    with pytest.raises(ValueError):
        bank.audit_of(["a", "b"], 0.5, 3, 3, tot, hist, sole, ov)


# ---- validation before any library call --------------------------------------------------------------------------------------------------------------------------------

class _StubLib(kk.StubLib):
    PREFIX = "mvb_"
    rounds = 0

    def mark(self, h, v, Q, th, first, count):
        self._thresholds(th, Q)
        self.log.append(("mark", Q, first, count))
        return 0

    def totals(self, h, out):
        self.log.append(("totals",))
        return 0

    def multiplicity(self, h, hist, sole, mult, sole_of):
        self.log.append(("multiplicity", mult is not None, sole_of is not None))
        return 0

    def overlap(self, h, out):
        self.log.append(("overlap",))
        return 0

    def greedy(self, h, w_pos, w_neg, fixed, max_rounds, rounds, order, gained):
        self.log.append(("greedy", w_pos, w_neg, fixed is not None, max_rounds))
        C.cast(rounds, C.POINTER(C.c_int))[0] = self.rounds
        return 0


W512 = kk.W512


def test_bad_arguments_raise_before_any_call():
    lib = _StubLib()
    for args in ((0, 500, W512, 0), (0, 512, W512, 2), (0, 512, W512[:, :100], 0), (0, 512, W512.astype(np.float64), 0), (-1, 512, W512, 0), (0, 512.0, W512, 0)):
        with pytest.raises((ValueError, TypeError)):
            bank.BankAudit(*args, lib=lib)
    assert lib.log == []
    with bank.BankAudit(0, 512, W512, 1, lib=lib) as ix:
        assert lib.log == [("create", 0, 512, 1)]
        ok = np.zeros((10, 512), np.float32)
        for bad in (ok.astype(np.float64), ok[:, :500], ok[:, ::2], ok.tolist(), ok[0]):
            with pytest.raises((ValueError, TypeError)):
                ix.add(bad)
        ix.add(ok)
        assert lib.log[-1] == ("add", 10) and len(ix) == 10
        v = np.zeros((3, 512), np.float32)
        n_calls = len(lib.log)
        for i, call in enumerate((lambda: ix.totals(), lambda: ix.multiplicity(), lambda: ix.overlap(), lambda: ix.greedy())):  # nothing marked yet
            with pytest.raises(RuntimeError, match="no marking is held"):
                call()
        calls = (lambda: ix.mark(v, [0.5, 0.6]), lambda: ix.mark(v, np.nan), lambda: ix.mark(v, "0.5"), lambda: ix.mark(v, True), lambda: ix.mark(v, 0.5, 3, 8),
                 lambda: ix.mark(v, 0.5, -1), lambda: ix.mark(v[:0], 0.5), lambda: ix.mark(v.astype(np.float64), 0.5), lambda: ix.mark(v, np.zeros(3, np.float16)),
                 lambda: ix.mark(np.zeros((4097, 512), np.float32), 0.5), lambda: ix.mark(np.zeros((3, 768), np.float32), 0.5), lambda: ix.mark(v.tolist(), 0.5),
                 lambda: ix.set_classes(np.zeros(11, np.uint8)), lambda: ix.set_classes(np.full(3, 2, np.uint8)), lambda: ix.set_classes(np.zeros(3, np.int64)),
                 lambda: ix.set_classes([0, 1]), lambda: ix.set_classes(np.zeros(3, np.uint8), -1))
        for i, call in enumerate(calls):
            with pytest.raises((ValueError, TypeError)):
                call()
            assert len(lib.log) == n_calls, i
        assert ix.mark(v, 0.51, 2) == (3, 8)
        assert lib.log[-1] == ("mark", 3, 2, 8) and lib.th.tolist() == [float(np.nextafter(np.float32(0.51), np.float32(1)))] * 3 and float(lib.th[0]) > 0.51
        ix.mark(v, np.float32(0.51))  # an fp32 number is its own threshold
        assert lib.th.tolist() == [float(np.float32(0.51))] * 3
        ix.mark(v, np.array([0.1, 0.2, 0.3]))
        assert lib.th.tobytes() == claims.up32([0.1, 0.2, 0.3]).tobytes()
        n_calls = len(lib.log)
        bad_greedy = (lambda: ix.greedy(-1), lambda: ix.greedy(1, 2 ** 20 + 1), lambda: ix.greedy(1.5), lambda: ix.greedy(max_rounds=-1), lambda: ix.greedy(fixed=[1, 0, 0]),
                      lambda: ix.greedy(fixed=np.zeros(4, np.uint8)), lambda: ix.greedy(fixed=np.zeros(3, np.int64)))
        for i, call in enumerate(bad_greedy):
            with pytest.raises((ValueError, TypeError)):
                call()
            assert len(lib.log) == n_calls, i
        t = ix.totals()
        h, s = ix.multiplicity()
        h2, s2, mult, sole_of = ix.multiplicity(per_row=True)
        ov = ix.overlap()
        assert t.shape == (3, 2) and h.shape == (2, 4) and s.shape == (3, 2) and ov.shape == (3, 3, 2) and all(a.dtype == np.int64 for a in (t, h, s, ov))
        assert mult.shape == sole_of.shape == (10,) and mult.dtype == np.uint16 and sole_of.dtype == np.int32
        assert lib.log[-4:] == [("totals",), ("multiplicity", False, False), ("multiplicity", True, True), ("overlap",)]
        lib.rounds = 2
        o, g = ix.greedy(3, 1, np.array([True, False, False]), 2)
        assert lib.log[-1] == ("greedy", 3, 1, True, 2) and o.shape == (2,) and o.dtype == np.int32 and g.shape == (2, 2) and g.dtype == np.int64
        lib.rounds = 0
        o, g = ix.greedy()
        assert lib.log[-1] == ("greedy", 1, 1, False, 3) and o.shape == (0,) and g.shape == (0, 2)
        for drop in (lambda: ix.set_classes(np.array([True, False, True]), 7), lambda: ix.test_plan(64, 5, 3), lambda: ix.add(ok), lambda: ix.reset()):
            ix.mark(v, 0.5)
            drop()
            with pytest.raises(RuntimeError, match="no marking is held"):
                ix.totals()
        assert ("classes", 7, 3) in lib.log and ("plan", 64, 5, 3) in lib.log and len(ix) == 0
        with pytest.raises(RuntimeError, match="stub"):
            ix.kernel_ms()
    assert lib.log[-1] == ("destroy",)
    with pytest.raises(RuntimeError, match="closed"):
        ix.mark(v, 0.5)


# ---- ModelMemory.anchor_bank_audit and the command line on the stand-in -------------------------------------------------------------------------------------------------

def _want_doc(ps, same, thres, labels, w_pos=1, w_neg=1):
    B = ps.astype(np.float64) >= np.asarray(thres, np.float64)[None, :]  # the reference's comparison: float(p32) >= t
    pred = B.any(1)
    TP, FP, FN, TN = int((pred & same).sum()), int((pred & ~same).sum()), int((~pred & same).sum()), int((~pred & ~same).sum())
    return B, dict(TP=TP, FP=FP, FN=FN, TN=TN)


def test_anchor_bank_audit_on_the_standin(standin_model):
    model, arrays, fx = standin_model
    _, _, ps = model.sweep_arrays(arrays, batch_size=8, with_probs=True, keep=True)
    ps = ps.astype(np.float32)
    same = np.asarray(arrays["same"], bool)
    thres = [float(np.percentile(ps[:, g], 70)) for g in range(4)]
    doc = model.anchor_bank_audit(arrays, thres, w_pos=2, w_neg=1, index_factory=_NumpyBank)
    B, union = _want_doc(ps, same, thres, model._golden_labels)
    assert 0 < B.sum() < B.size and {k: doc["union"][k] for k in union} == union and doc["rows"] == 23 and doc["positives"] == int(same.sum())
    assert set(doc) == {"rows", "positives", "union", "anchors", "overlaps", "greedy"} and set(doc["union"]) == {"TP", "FP", "FN", "TN", "precision", "recall", "f1"}
    assert [a["anchor"] for a in doc["anchors"]] == model._golden_labels == [f"CWE-{100 + i}" for i in range(4)] and [a["thres"] for a in doc["anchors"]] == thres
    for g, a in enumerate(doc["anchors"]):
        assert set(a) == {"anchor", "thres", "claimed", "sole", "f1_without"}
        assert a["claimed"] == [int((B[:, g] & ~same).sum()), int((B[:, g] & same).sum())]
        only = B[:, g] & (B.sum(1) == 1)
        assert a["sole"] == [int((only & ~same).sum()), int((only & same).sum())]
        rest = np.delete(B, g, 1).any(1)  # the bank without it, computed from scratch
        tp, fp, fn = int((rest & same).sum()), int((rest & ~same).sum()), int((~rest & same).sum())
        assert a["f1_without"] == pytest.approx(2 * tp / (2 * tp + fp + fn) if tp else 0.0)
    for o in doc["overlaps"]:
        q, r = model._golden_labels.index(o["a"]), model._golden_labels.index(o["b"])
        both = B[:, q] & B[:, r]
        assert q < r and o["both"] == [int((both & ~same).sum()), int((both & same).sum())] and o["jaccard"] == pytest.approx(both.sum() / (B[:, q] | B[:, r]).sum())
    assert [o["jaccard"] for o in doc["overlaps"]] == sorted((o["jaccard"] for o in doc["overlaps"]), reverse=True) and len(doc["overlaps"]) <= 6
    order, gained, _ = kit.greedy(B, same.astype(np.uint8), 2, 1)
    assert [g["index"] for g in doc["greedy"]] == order.tolist() and [[g["new_pos"], g["new_neg"]] for g in doc["greedy"]] == gained.tolist()
    assert [g["TP"] for g in doc["greedy"]] == np.cumsum(gained[:, 0]).tolist() and [g["FP"] for g in doc["greedy"]] == np.cumsum(gained[:, 1]).tolist()
    json.dumps(doc)
    ix = _NumpyBank.made[0]
    assert len(_NumpyBank.made) == 1 and np.array_equal(ix.w, fx[4]["_projector.weight"]) and ix.u.shape == (23, 512) and np.array_equal(ix.cls, same.astype(np.uint8))
    # one download serves the three indexes
    assert _CountingEngine.downloads == 1
    model.anchor_claims(arrays, 0.5, index_factory=_NumpyClaims)
    model.anchor_reports(arrays, 3, index_factory=_NumpyIndex)
    assert _CountingEngine.downloads == 1 and model._kept.embed is None
    # candidates: the bank is fixed, the candidates are ranked by what they add
    cand = np.ascontiguousarray(model.engine.anchor_get()[[2, 0]] * np.float32(0.5))
    lo = float(np.percentile(ps, 40))
    doc2 = model.anchor_bank_audit(arrays, thres, candidates=cand, candidate_labels=["fresh", "other"], candidate_thres=lo, w_pos=2, w_neg=1, index_factory=_NumpyBank)
    assert len(_NumpyBank.made) == 1 and {k: doc2["union"][k] for k in union} == union and doc2["anchors"] == doc["anchors"]
    from oracle import memvul_oracle as orc

    _, pc, _, _ = orc.match(ix.u, cand, ix.w, ix.same_idx)
    Bc = pc[:, :, ix.same_idx].astype(np.float32).astype(np.float64) >= lo
    order2, gained2, _ = kit.greedy(np.concatenate([B, Bc], 1), same.astype(np.uint8), 2, 1, np.array([1, 1, 1, 1, 0, 0]))
    assert [g["index"] for g in doc2["greedy"]] == (order2 - 4).tolist() and [g["anchor"] for g in doc2["greedy"]] == [["fresh", "other"][i - 4] for i in order2]
    assert [[g["new_pos"], g["new_neg"]] for g in doc2["greedy"]] == gained2.tolist()
    if len(order2):
        assert doc2["greedy"][0]["TP"] == union["TP"] + int(gained2[0, 0]) and doc2["greedy"][0]["FP"] == union["FP"] + int(gained2[0, 1])
    assert [c["anchor"] for c in doc2["candidates"]] == ["fresh", "other"] and [c["claimed"] for c in doc2["candidates"]] == [
        [int((Bc[:, i] & ~same).sum()), int((Bc[:, i] & same).sum())] for i in range(2)]
    for bad in (dict(thres=[0.5, 0.5]), dict(thres=float("nan")), dict(candidates=cand, candidate_labels=["one"])):
        with pytest.raises(ValueError):
            model.anchor_bank_audit(arrays, index_factory=_NumpyBank, **{"thres": thres, **bad})
    # a new sweep drops the index with the other two
    model.sweep_arrays(arrays, 4, 20, batch_size=8, with_probs=True, keep=True)
    assert ix.closed and model._kept.indexes["bank"] is None
    doc3 = model.anchor_bank_audit(arrays, thres, 4, 20, index_factory=_NumpyBank)
    assert len(_NumpyBank.made) == 2 and _NumpyBank.made[1].u.shape == (16, 512) and np.array_equal(_NumpyBank.made[1].cls, same[4:20].astype(np.uint8))
    assert doc3["rows"] == 16 and doc3["positives"] == int(same[4:20].sum())


def test_the_command_line_writes_one_json_document(capsys, tmp_path):
    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=12, n_anchors=4, layers=2)
    try:
        _KeepingEngine.created, _NumpyBank.made = [], []
        out = tmp_path / "bank.json"
        std = ["--archive", arch, "--golden", golden, "--input", test_path]
        rc = bank.main(std + ["--thres", "0.0", "--out", str(out)], engine_factory=_KeepingEngine, index_factory=_NumpyBank)
        doc = json.load(open(out))
        assert rc == 0 and capsys.readouterr().out.strip() == "" and _NumpyBank.made[0].closed
        assert doc["rows"] == 12 and doc["union"]["FN"] == 0 and doc["union"]["TN"] == 0 and [a["anchor"] for a in doc["anchors"]] == [f"CWE-{100 + i}" for i in range(4)]
        assert all(sum(a["claimed"]) == 12 and a["sole"] == [0, 0] for a in doc["anchors"]) and all(o["jaccard"] == 1.0 for o in doc["overlaps"]) and len(doc["overlaps"]) == 6
        eng = _KeepingEngine.created[0]
        ids, lens, _ = _inputs(arch, golden, test_path)
        ps = eng.forward(ids, lens)["probs"][:, :, 0].astype(np.float32)
        same = _NumpyBank.made[0].cls.astype(bool)
        per = {"CWE-101": float(np.percentile(ps[:, 1], 60)), "CWE-103": float(np.percentile(ps[:, 3], 30))}
        tf = tmp_path / "thres.json"
        tf.write_text(json.dumps(per))
        mid = float(np.median(ps))
        rc = bank.main(std + ["--thres", repr(mid), "--thres-file", str(tf), "--top", "2", "--w-pos", "3", "--max-rounds", "2"], engine_factory=_KeepingEngine,
                       index_factory=_NumpyBank)
        doc = json.loads(capsys.readouterr().out)
        thres = [mid, per["CWE-101"], mid, per["CWE-103"]]
        B, union = _want_doc(ps, same, thres, None)
        assert rc == 0 and [a["thres"] for a in doc["anchors"]] == thres and {k: doc["union"][k] for k in union} == union and len(doc["overlaps"]) <= 2
        order, gained, _ = kit.greedy(B, same.astype(np.uint8), 3, 1, None, 2)
        assert [g["index"] for g in doc["greedy"]] == order.tolist() and len(doc["greedy"]) <= 2
        tf.write_text(json.dumps({"CWE-999": 0.5}))
        for bad in (["--thres", "nan"], ["--w-pos", "-1"], ["--w-neg", str(2 ** 20 + 1)], ["--top", "-1"], ["--thres-file", str(tf)]):
            with pytest.raises(SystemExit):
                bank.main(std + bad, engine_factory=_KeepingEngine, index_factory=_NumpyBank)
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- no GPU, no index -------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_constructor_raises_without_a_gpu(libs):
    try:
        has_gpu = subprocess.run(["/opt/rocm/bin/rocm_agent_enumerator"], capture_output=True, text=True).stdout.count("gfx9") > 0
    except Exception:
        has_gpu = False
    with pytest.raises(RuntimeError, match="mvb_create"):
        bank.BankAudit(4096 if has_gpu else 0, 512, W512, 0)  # (with a GPU: a device that is not there)
    with pytest.raises(RuntimeError, match="not found"):
        bank.load_library(os.path.join(ROOT, "memvul_amd", "lib", "no_such_library.so"))
