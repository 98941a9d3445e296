"""The sink census without a GPU: the ABI, the strict switch, the committed fixture, and a numpy restatement of the kernel's bookkeeping (tests/census_kit.py
census_numpy) that passes the GPU test's checks on the fixture as written — and fails them with each of four planted mistakes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import census_kit as ck  # noqa: E402
import make_sink_census_refs as mk  # noqa: E402
from memvul_amd import binding, synth  # noqa: E402

V = mk.DIMS["vocab_size"]
NAMES = ("mv_sink_census_enable", "mv_sink_census_read")
MISTAKES = ("drop_map", "gate_gt", "exclude_last_row", "tie_high")


@pytest.fixture(scope="module")
def refs(golden_dir):
    r = np.load(os.path.join(golden_dir, "sink_census_refs.npz"))
    return {k: r[k] for k in r.files}


@pytest.fixture(scope="module")
def delta_abs(golden_dir):
    return float(np.load(os.path.join(golden_dir, "monitor_refs.npz"))["delta_abs"])


def test_header_and_binding_declare_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    assert re.search(r"\bint mv_sink_census_enable\(mv_handle\* h, int on\);", hdr)
    assert re.search(r"\bint mv_sink_census_read\(mv_handle\* h, uint32_t\* items, uint64_t\* share_q20, int vocab, uint32_t\* by_head, int layers_x_heads, int reset\);", hdr)
    for name in NAMES:
        assert name in binding.ABI_SYMBOLS
    from stage_kit import host_source

    src = host_source()
    for name in NAMES:  # function-try-blocks, like every entry point
        assert re.search(r"^int %s\([^{;]*\) try \{" % name, src, flags=re.M), name
    assert "sink_census.h" in open(os.path.join(ROOT, "memvul_amd", "build.py")).read()  # (a kernel edit must move the build's fingerprint)


def test_the_built_library_exports_them():
    if not os.path.exists(binding.LIB_PATH):
        pytest.skip("libmemvul_hip.so not built")
    lib = binding.load_library()
    assert lib.mv_sink_census_enable.argtypes == [C.c_void_p, C.c_int] and lib.mv_sink_census_enable.restype == C.c_int
    assert lib.mv_sink_census_read.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    assert lib.mv_sink_census_read(None, None, None, 0, None, 0, 0) == -1 and lib.mv_sink_census_enable(None, 1) == -1  # (MV_ERR_INVALID: no handle)


def test_the_switch_is_parsed_strictly(monkeypatch):
    monkeypatch.delenv("MEMVUL_SINK_CENSUS", raising=False)
    assert binding.sink_census_policy() is False
    for v, want in (("0", False), ("1", True)):
        monkeypatch.setenv("MEMVUL_SINK_CENSUS", v)
        assert binding.sink_census_policy() is want
    for v in ("", "yes", "true", "2", " 1", "on"):
        monkeypatch.setenv("MEMVUL_SINK_CENSUS", v)
        with pytest.raises(ValueError, match="MEMVUL_SINK_CENSUS"):
            binding.sink_census_policy()
        with pytest.raises(ValueError, match="MEMVUL_SINK_CENSUS"):  # before anything is created
            binding.Engine(0)


def test_the_committed_fixture_holds_its_own_conditions(refs):
    """m from the stored rounding-model gaps, uncertain items <= 5 % of the possibly-over items of every case, the controls empty, every sink kind present."""
    m = mk.check(refs, verbose=False)
    assert m == float(refs["m"]) and 0 < m < 0.05
    for name in mk.MODELS:
        assert int(refs[name + "_seed"]) == mk.MODELS[name][3]


# the cases the restatement runs on: the exact float64 rows are computed here (seconds at these sizes) and must reproduce the committed arrays
CASES = (("two_tok", 64), ("ord_80", 64))


@pytest.fixture(scope="module")
def exact_rows(refs):
    out = {}
    for model, W in CASES:
        ids, lens, names = mk.case_inputs(model, W)
        p = ck.cls_rows(mk.weights(model, refs[model + "_gains"]), ids, lens)
        s = ck.summarise(p, lens)
        for k in mk.KEYS:
            a, b = s[k], refs["%s_%d_%s" % (model, W, k)]
            assert np.array_equal(a, b) if k.startswith("pos") else np.allclose(a, b, rtol=0, atol=1e-12), (model, W, k)
        out[model, W] = (p, ids, lens, names)
    return out


def _tie_case():
    """A hand-made case for the tie: one 20-token sequence, one layer, one head, two DIFFERENT tokens with exactly equal shares of 0.45 at positions 5 and 12."""
    n = 20
    p = np.full((1, 1, 1, n), 0.1 / (n - 2))
    p[..., 5] = p[..., 12] = 0.45
    ids = np.arange(1000, 1000 + n, dtype=np.int32)[None]
    ids[0, 0], ids[0, n - 1] = synth.CLS_ID, synth.SEP_ID
    ref = ck.summarise(p, [n])
    assert ref["pos1"][0, 0, 0] == 5 and ref["pos2"][0, 0, 0] == 12  # (the reference's own tie goes to the lowest position)
    return p, ids, np.array([n], np.int32), ref


def _failures(refs, delta_abs, exact_rows, **mistake):
    m = float(refs["m"])
    bad = []
    for (model, W), (p, ids, lens, _) in exact_rows.items():
        for layers in (2, 3):
            bd = ck.bounds(mk.case_ref(refs, model, W), ids, lens, layers, V, delta_abs, m)
            bad += ck.check_census(ck.census_numpy(p[:layers], ids, lens, V, **mistake), bd, m, f"{model} {W} {layers}")[0]
    p, ids, lens, ref = _tie_case()
    bd = ck.bounds(ref, ids, lens, 1, V, delta_abs, 0.0)  # (m = 0: an exact tie is decided by the rule, not by a margin)
    bad += ck.check_census(ck.census_numpy(p, ids, lens, V, **mistake), bd, 2.0 ** -20, "tie")[0]  # (the share itself: to the q20 grid)
    return bad


def test_the_restatement_passes_the_gpu_tests_checks(refs, delta_abs, exact_rows):
    """The engine row order, rows >= 2, the map back to the token position, the lowest-position tie, the 16-token gate and the q20 rounding, in numpy."""
    assert _failures(refs, delta_abs, exact_rows) == []
    # what the planted mistakes need is in these cases: the sink at position 1, a 16-token row over the threshold, both sink tokens
    p, ids, lens, names = exact_rows["two_tok", 64]
    items = ck.census_numpy(p, ids, lens, V)[0]
    assert items[synth.MID_ID] > 0 and items[mk.SECOND_ID] > 0
    hit16 = hit_first = False
    for (model, W), (p, ids, lens, names) in exact_rows.items():
        one = lambda b: ck.census_numpy(p[:, b:b + 1], ids[b:b + 1], lens[b:b + 1], V)[0].sum()  # noqa: E731
        hit16 |= one(3) > 0
        hit_first |= any(one(b) > 0 for b, k in enumerate(names) if k == "first" and lens[b] >= 16)
    assert hit16 and hit_first
    assert ck.census_numpy(*_tie_case()[:3], V)[1][1005] == int(np.rint(np.float32(0.45) * np.float32(ck.Q20)))


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_checks_notice_each_planted_mistake(refs, delta_abs, exact_rows, mistake):
    """The row-to-position map dropped, > 16 instead of >= 16, key len - 1 excluded instead of row 1, the tie broken toward the highest position."""
    bad = _failures(refs, delta_abs, exact_rows, **{mistake: True})
    assert bad, mistake
    print(mistake, len(bad), bad[0])
