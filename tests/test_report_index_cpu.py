"""Per-anchor retrieval (memvul_amd/retrieve.py, libmemvul_retrieve.so): what needs no GPU — the names, the build, the built kernels' resources, the plan in numpy
against the order it must produce, the Python validation on a recording stub, and ModelMemory.anchor_reports / the command line on the oracle-backed stand-in."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from memvul_amd import build, retrieve

import kept_index_kit as kk
import plumbing_util as pu
import report_index_kit as kit
from kept_index_kit import _KeepingEngine, _NumpyIndex, _inputs, standin_model  # noqa: F401  (standin_model is a fixture)
import test_corpus_rematch_cpu as rm
from test_f32_form_cpu import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "memvul_amd", "csrc")
NEW_KERNELS = ("report_weight_delta_kernel", "report_row_term_kernel", "report_query_prep_kernel", "report_score_kernel", "report_merge_kernel")


@pytest.fixture(scope="module")
def libs():
    paths = build.build_all(verbose=False)
    return paths


# ---- 1, 2: the names and the exception rule ---------------------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "memvul_retrieve.h")).read(), flags=re.S)


def test_header_binding_and_library_agree(libs):
    declared = sorted(set(re.findall(r"\b(mvr_[a-z_0-9]+)\s*\(", _header())))
    assert declared == sorted(retrieve.RETRIEVE_SYMBOLS) and len(declared) == 10
    lib = retrieve.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libmemvul_retrieve.so does not export {name}"


def test_no_cpp_exception_can_cross_the_boundary():
    src = open(os.path.join(CSRC, "retrieve.hip")).read()
    heads = re.findall(r"^int (mvr_\w+)\(([^{;]*?)\)\s*(try\s*)?\{", src, flags=re.M)
    declared = sorted(set(re.findall(r"^\s*int\s+(mvr_\w+)\s*\(", _header(), flags=re.M)))
    assert len(declared) == 7 and sorted(name for name, _, _ in heads) == declared
    assert all(guard for _, _, guard in heads), [name for name, _, guard in heads if not guard]
    assert src.count("catch (...) { return on_exception(") == len(heads)


# ---- 3, 4: the build --------------------------------------------------------------------------------------------------------------------------------------------

def test_build_all_returns_two_paths_and_leaves_three_fresh_libraries(libs):
    assert list(libs) == [build.LIB_PATH, build.LIB_PATH_DEV]
    assert not build.is_stale() and not build.is_stale(dev=True) and not build.retrieve_is_stale() and not build.tok_is_stale()
    assert os.path.exists(build.LIB_PATH_RETRIEVE) and os.path.basename(build.LIB_PATH_RETRIEVE) == build.RETRIEVE_LIB_NAME == "libmemvul_retrieve.so"


def test_the_kernels_are_the_recorded_ones(libs):
    kk.check_kernels_are_the_recorded_ones(build.LIB_PATH_RETRIEVE, "retrieve")


def test_the_main_library_does_not_know_the_new_files(libs, monkeypatch):
    new, _ = kk.own_and_shared("retrieve")
    assert sorted(os.path.basename(p) for p in new) == ["memvul_retrieve.h", "report_topk.h", "retrieve.hip"]
    assert build.SIDE_LIBS["retrieve"] == (build.RETRIEVE_LIB_NAME, build.RETRIEVE_SOURCES, build.RETRIEVE_HEADERS)
    kk.check_the_shared_headers_belong_to_the_four_kept_libraries(monkeypatch)
    opened = []
    real_open = open

    def spy(path, *a, **kw):
        opened.append(os.path.abspath(path) if isinstance(path, str) else path)
        return real_open(path, *a, **kw)

    monkeypatch.setattr("builtins.open", spy)
    build.source_fingerprint()
    for other in ("tok", "claims", "bank"):
        build.source_fingerprint((), *build.SIDE_LIBS[other][1:])
    monkeypatch.undo()
    assert opened and not set(opened) & set(new)
    for name in os.listdir(CSRC):  # nothing the main library is built from includes the new header
        if name not in ("retrieve.hip", "report_topk.h"):
            assert "report_topk.h" not in open(os.path.join(CSRC, name)).read(), name
    src = open(os.path.join(CSRC, "retrieve.hip")).read() + open(os.path.join(CSRC, "report_topk.h")).read()
    assert not re.search(r'#include\s+"match_topk.h"', src)
    main, new_map = build.kernel_fingerprints(build.LIB_PATH), build.kernel_fingerprints(build.LIB_PATH_RETRIEVE)
    assert not [k for k in main if any(n in k for n in NEW_KERNELS)]
    for n in NEW_KERNELS:
        assert any(n in k and k.endswith(".kd") for k in new_map), n
    assert not [k for k in new_map if "match_topk_kernel" in k or "topk_merge_kernel" in k or "rematch_merge_kernel" in k]
    assert not set(new_map) & set(main)


# ---- 5: the code object -----------------------------------------------------------------------------------------------------------------------------------------

def test_no_kernel_uses_scratch_or_atomics_and_lds_stays_within_the_cu(libs, tmp_path):
    (co,) = build.device_code_objects(build.LIB_PATH_RETRIEVE)
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
    assert len([k for k in kernels if "report_score_kernel" in k]) == 16  # P 512 / 768 x 64 / 128 / 256 / 512 rows per block x ranking / P(same)
    for k, (scratch, lds, spill) in kernels.items():
        assert scratch == 0 and spill == 0 and lds <= 160 * 1024, (k, scratch, lds, spill)
    asm = subprocess.run([_llvm_tool("llvm-objdump"), "-d", str(elf)], capture_output=True, text=True, check=True).stdout
    mnemonics = set(re.findall(r"^\s+([a-z_0-9]+) ", asm, flags=re.M))  # (the first line names the file: only the instruction column is searched)
    assert "v_fma_f32" in mnemonics and not [m for m in mnemonics if m.startswith("scratch_") or "atomic" in m]
    score = subprocess.run([_llvm_tool("llvm-objdump"), "-d", "--disassemble-symbols=" + next(k for k in kernels if "report_score_kernelILi512ELi256ELi0" in k), str(elf)],
                           capture_output=True, text=True, check=True).stdout
    # the chains stay on the plain forms: |x| as a source modifier of v_fma_f32, no packed pair with a v_and per value (report_topk.h RT_OPAQUE16)
    assert len(re.findall(r"v_fma_f32 v\d+, s\d+, \|v\d+\|, v\d+", score)) >= 128 and "v_pk_fma_f32" not in score


# ---- 6: the plan in numpy ---------------------------------------------------------------------------------------------------------------------------------------

Q_PLAN = 7


@pytest.fixture(scope="module")
def tie_heavy():
    """P(same) [4099, 7] of the fixture, quantised to 1/32 so that MANY rows tie, with a NaN row; computed once."""
    U, V, W = kit.fixture(11, 4099, 64, Q_PLAN)
    p = (np.round(kit.psame_f64(U, V, W, 0) * 32) / 32).astype(np.float32)
    p[1234, 2] = np.float32("nan")
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("block_rows", [64, 256])
@pytest.mark.parametrize("fan_in", [2, 3, 16])
@pytest.mark.parametrize("anchor_group", [1, 5, Q_PLAN])
def test_the_plan_gives_the_reference_order(tie_heavy, N, block_rows, fan_in, anchor_group):
    p = tie_heavy[:N]
    for k in (1, 10, 64):  # (k > N at the small sizes)
        want_p, want_r = kit.reference_topk(p, k)
        got_p, got_r = kit.plan_model(p, k, block_rows, fan_in, anchor_group)
        assert np.array_equal(got_r, want_r) and got_p.tobytes() == want_p.tobytes(), (N, k)
    if N == 4099:
        assert kit.merge_levels(N, 64, 2) >= 6


def test_the_reference_order_by_hand():
    p = np.array([[0.5, 0.1], [0.9, np.nan], [0.5, 0.1], [0.9, 0.3]], np.float32)
    tp, tr = kit.reference_topk(p, 5, first=10)
    assert tr.tolist() == [[11, 13, 10, 12, -1], [11, 13, 10, 12, -1]]
    assert tp[0].tolist() == [np.float32(0.9), np.float32(0.9), 0.5, 0.5, -1.0] and np.isnan(tp[1, 0]) and tp[1, 4] == -1.0
    tp0, tr0 = kit.reference_topk(np.zeros((0, 2), np.float32), 3)
    assert (tr0 == -1).all() and (tp0 == -1).all()


@pytest.mark.parametrize("fault", ["tie_high", "short_list", "drop_last", "no_offset"])
def test_the_plan_model_sees_each_seeded_fault(tie_heavy, fault):
    p = tie_heavy[:257]
    want_p, want_r = kit.reference_topk(p, 10)
    got_p, got_r = kit.plan_model(p, 10, 64, 2, 5, fault=fault)
    assert not np.array_equal(got_r, want_r)


# ---- 7: validation before any library call ------------------------------------------------------------------------------------------------------------------------

class _StubLib(kk.StubLib):
    PREFIX = "mvr_"

    def query(self, h, v, Q, k, first, count, p, r):
        self.log.append(("query", Q, k, first, count))
        return 0

    def psame(self, h, v, Q, first, count, p):
        self.log.append(("psame", Q, first, count))
        return 0


W512 = kk.W512


def test_bad_arguments_raise_before_any_call():
    lib = _StubLib()
    for args in ((0, 500, W512, 0), (0, 512, W512, 2), (0, 512, W512[:, :100], 0), (0, 512, W512.astype(np.float64), 0), (-1, 512, W512, 0), (0, 512.0, W512, 0)):
        with pytest.raises((ValueError, TypeError)):
            retrieve.ReportIndex(*args, lib=lib)
    assert lib.log == []
    with retrieve.ReportIndex(0, 512, W512, 1, lib=lib) as ix:
        assert lib.log == [("create", 0, 512, 1)]
        ok = np.zeros((10, 512), np.float32)
        bad_rows = (ok.astype(np.float64), ok[:, :500], ok[:, ::2], np.zeros((10, 1024), np.float32)[:, ::2], ok.tolist(), ok[0])
        for bad in bad_rows:
            with pytest.raises((ValueError, TypeError)):
                ix.add(bad)
        assert len(lib.log) == 1
        ix.add(ok)
        assert lib.log[-1] == ("add", 10) and len(ix) == 10
        n_calls = len(lib.log)
        v = np.zeros((3, 512), np.float32)
        for call in (lambda: ix.query(v, 0), lambda: ix.query(v, 65), lambda: ix.query(v, 1.5), lambda: ix.query(v, 3, -1), lambda: ix.query(v, 3, 5, 6),
                     lambda: ix.query(v, 3, 11), lambda: ix.query(v, 3, 0, -1), lambda: ix.query(v[:0], 3), lambda: ix.query(np.zeros((4097, 512), np.float32), 3),
                     lambda: ix.query(v.astype(np.float16), 3), lambda: ix.query(np.zeros((3, 768), np.float32), 3), lambda: ix.query(np.asfortranarray(v), 3),
                     lambda: ix.psame(v, 0, 11), lambda: ix.psame(v[:0]), lambda: ix.psame(v.astype(np.float64))):
            with pytest.raises((ValueError, TypeError)):
                call()
        assert len(lib.log) == n_calls
        lib.n = 2 ** 28  # (the stub only counts)
        with pytest.raises(ValueError, match="2\\^28"):
            ix.psame(v[:2])
        with pytest.raises(ValueError, match="2\\^31"):
            lib.n = 2 ** 31 - 5
            ix.add(ok)
        assert len(lib.log) == n_calls
        lib.n = 10
        p, r = ix.query(v, 4, 2)
        assert lib.log[-1] == ("query", 3, 4, 2, 8) and p.shape == (3, 4) and p.dtype == np.float32 and r.dtype == np.int64
        assert ix.psame(v, 1, 3).shape == (3, 3) and lib.log[-1] == ("psame", 3, 1, 3)
        with pytest.raises(RuntimeError, match="stub"):
            ix.kernel_ms()
        ix.reset()
        assert len(ix) == 0
    assert lib.log[-1] == ("destroy",)
    with pytest.raises(RuntimeError, match="closed"):
        ix.query(v, 3)


class _EmbedLib(rm._Lib):
    """The recorder of the rematch tests plus mv_corpus_embeddings: every row carries its row number of the UPLOAD."""

    def mv_corpus_embeddings(self, h, first, count, out):
        self.log.append(("embeddings", first, count))
        o = C.cast(out, C.POINTER(C.c_float))
        for r in range(count):
            o[r * 512] = float(first + r)
        return 0


class _RecIndex:
    made = []

    def __init__(self, device, P, w, same_idx):
        self.args, self.rows, self.closed = (device, P, same_idx), [], False
        _RecIndex.made.append(self)

    def add(self, e):
        assert e.dtype == np.float32 and e.flags["C_CONTIGUOUS"]
        self.rows.append(e[:, 0].copy())

    def close(self):
        self.closed = True


def test_from_sweep_delivers_the_rows_in_the_original_order(monkeypatch):
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    lib = _EmbedLib(sink_share=0.0)
    eng = rm.sf.StandInEngine(lib)
    eng.device = 0
    eng.anchor_append(rm.sf.IDS[:5], rm.sf.LENS[:5])
    with pytest.raises(RuntimeError, match="keep=True"):
        eng.sweep_embeddings()
    eng.bucketed_sweep(rm.sf.IDS, rm.LENS, 4, topk=2)  # top-k lists, no embeddings
    with pytest.raises(RuntimeError, match="keep=True"):
        retrieve.ReportIndex.from_sweep(eng, W512, 0, index_factory=_RecIndex)
    eng.bucketed_sweep(rm.sf.IDS, rm.LENS, 4, keep=True)
    order = np.argsort(rm.LENS, kind="stable")  # original row order[j] is row j of the upload
    inv = np.argsort(order)
    e = eng.sweep_embeddings()
    assert e.shape == (8, 512) and e[:, 0].tolist() == inv.tolist()
    assert eng.sweep_embeddings(2, 3, chunk=2)[:, 0].tolist() == inv[2:5].tolist() and eng.sweep_embeddings(8, 0).shape == (0, 512)
    with pytest.raises(ValueError):
        eng.sweep_embeddings(5, 4)
    _RecIndex.made = []
    n0 = len(lib.log)
    ix = retrieve.ReportIndex.from_sweep(eng, W512, 0, chunk=3, index_factory=_RecIndex)
    assert ix is _RecIndex.made[0] and ix.args == (0, 512, 0) and [len(r) for r in ix.rows] == [3, 3, 2]
    assert np.concatenate(ix.rows).tolist() == inv.tolist()
    assert [c for c in lib.log[n0:]] == [("embeddings", 0, 3), ("embeddings", 3, 3), ("embeddings", 6, 2)]  # one pass over the upload, nothing else


# ---- 8: ModelMemory.anchor_reports and the command line on the stand-in ------------------------------------------------------------------------------------------

def test_anchor_reports_on_the_standin(standin_model):
    model, arrays, fx = standin_model
    w = fx[4]
    _, _, ps = model.sweep_arrays(arrays, batch_size=8, with_probs=True, keep=True)
    out = model.anchor_reports(arrays, 5, index_factory=_NumpyIndex)
    assert [e["anchor"] for e in out] == model._golden_labels == [f"CWE-{100 + i}" for i in range(4)]
    want_p, want_r = kit.reference_topk(ps.astype(np.float32), 5)
    for g, e in enumerate(out):
        assert [r["row"] for r in e["reports"]] == want_r[g].tolist()
        assert [r["Issue_Url"] for r in e["reports"]] == [arrays["urls"][r] for r in want_r[g]]
        assert [r["prob"] for r in e["reports"]] == pytest.approx(want_p[g].tolist(), abs=1e-6) and set(e["reports"][0]) == {"Issue_Url", "row", "prob"}
    json.dumps(out)
    assert len(_NumpyIndex.made) == 1 and np.array_equal(_NumpyIndex.made[0].w, w["_projector.weight"]) and _NumpyIndex.made[0].u.shape == (23, 512)
    # the same kept sweep: the index is reused; given vectors take their labels from labels=
    v = model.engine.anchor_get()[[2, 0]]
    out2 = model.anchor_reports(arrays, 3, vectors=v, labels=["fresh CVE", "another"], index_factory=_NumpyIndex)
    assert len(_NumpyIndex.made) == 1 and _NumpyIndex.made[0].queries == 2
    assert [e["anchor"] for e in out2] == ["fresh CVE", "another"] and [r["row"] for r in out2[0]["reports"]] == want_r[2, :3].tolist()
    assert [e["anchor"] for e in model.anchor_reports(arrays, 1, vectors=v, index_factory=_NumpyIndex)] == ["0", "1"]
    # k beyond the rows: the exhausted slots are left out
    assert [len(e["reports"]) for e in model.anchor_reports(arrays, 64, index_factory=_NumpyIndex)] == [23] * 4
    # a new sweep replaces the index: of rows 4 .. 20 now, numbered as in `arrays`
    first_index = _NumpyIndex.made[0]
    _, _, ps = model.sweep_arrays(arrays, 4, 20, batch_size=8, with_probs=True, keep=True)
    assert first_index.closed
    out3 = model.anchor_reports(arrays, 4, 4, 20, index_factory=_NumpyIndex)
    assert len(_NumpyIndex.made) == 2 and _NumpyIndex.made[1].u.shape == (16, 512)
    want_p, want_r = kit.reference_topk(ps.astype(np.float32), 4, first=4)
    assert [[r["row"] for r in e["reports"]] for e in out3] == want_r.tolist()
    assert [r["Issue_Url"] for r in out3[1]["reports"]] == [arrays["urls"][r] for r in want_r[1]]


def test_the_command_line_writes_one_json_line_per_anchor(capsys, tmp_path):
    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=12, n_anchors=4, layers=2)
    try:
        _KeepingEngine.created, _NumpyIndex.made = [], []
        out = tmp_path / "reports.jsonl"
        rc = retrieve.main(["--archive", arch, "--golden", golden, "--input", test_path, "--k", "3", "--out", str(out)], engine_factory=_KeepingEngine,
                           index_factory=_NumpyIndex)
        lines = [json.loads(ln) for ln in open(out)]
        assert rc == 0 and [e["anchor"] for e in lines] == [f"CWE-{100 + i}" for i in range(4)] and all(len(e["reports"]) == 3 for e in lines)
        eng = _KeepingEngine.created[0]
        ids, lens, arrs = _inputs(arch, golden, test_path)
        urls = arrs["urls"]
        p = eng.forward(ids, lens)["probs"][:, :, 0]
        want_p, want_r = kit.reference_topk(p.astype(np.float32), 3)
        assert sorted(urls) == sorted(r["Issue_Url"] for r in json.load(open(test_path)))  # (the reader's order, which "row" counts in, is its own)
        assert [[r["row"] for r in e["reports"]] for e in lines] == want_r.tolist()
        assert [r["Issue_Url"] for r in lines[2]["reports"]] == [urls[r] for r in want_r[2]]
        assert _NumpyIndex.made[0].closed and capsys.readouterr().out.strip() == ""
        rc = retrieve.main(["--archive", arch, "--golden", golden, "--input", test_path, "--k", "2", "--anchors", "CWE-102,CWE-100"], engine_factory=_KeepingEngine,
                           index_factory=_NumpyIndex)
        printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert rc == 0 and [e["anchor"] for e in printed] == ["CWE-102", "CWE-100"] and [r["row"] for r in printed[0]["reports"]] == want_r[2, :2].tolist()
        with pytest.raises(SystemExit):
            retrieve.main(["--archive", arch, "--golden", golden, "--input", test_path, "--anchors", "CWE-999"], engine_factory=_KeepingEngine, index_factory=_NumpyIndex)
        with pytest.raises(SystemExit):
            retrieve.main(["--archive", arch, "--golden", golden, "--input", test_path, "--k", "65"], engine_factory=_KeepingEngine, index_factory=_NumpyIndex)
    finally:
        shutil.rmtree(root, ignore_errors=True)


# ---- 9: no GPU, no index ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_constructor_raises_without_a_gpu(libs):
    try:
        has_gpu = subprocess.run(["/opt/rocm/bin/rocm_agent_enumerator"], capture_output=True, text=True).stdout.count("gfx9") > 0
    except Exception:
        has_gpu = False
    if has_gpu:
        with pytest.raises(RuntimeError, match="mvr_create"):  # a device that is not there
            retrieve.ReportIndex(4096, 512, W512, 0)
    else:
        with pytest.raises(RuntimeError, match="mvr_create"):
            retrieve.ReportIndex(0, 512, W512, 0)
    with pytest.raises(RuntimeError, match="not found"):
        retrieve.load_library(os.path.join(ROOT, "memvul_amd", "lib", "no_such_library.so"))
