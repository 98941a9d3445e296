"""Compute dtype "f32" (include/memvul_hip.h MV_F32, the reference form) and the contract audit built on it (memvul_amd/audit.py): what needs no GPU —
the names, the statistics, the audit's flow on the oracle-backed stand-in engine, the command line, and the built GEMM kernel's code."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from memvul_amd import audit, binding, build

import plumbing_util as pu


# ---- the names --------------------------------------------------------------------------------------------------------------------------------------------------

def test_compute_dtype_names():
    assert binding.compute_dtype_of("f32") == binding.compute_dtype_of("reference") == binding.compute_dtype_of(0) == binding.MV_F32 == 0
    assert binding.compute_dtype_of("F32") == 0
    assert binding.wanted_form("f32") is None
    for bad in ("bf16", 5, 2):
        with pytest.raises(ValueError):
            binding.compute_dtype_of(bad)
    assert binding.DEFAULT_COMPUTE == "precise"


def test_environment_selects_the_reference_form(monkeypatch):
    monkeypatch.setenv("MEMVUL_COMPUTE", "f32")
    assert binding.default_compute() == "f32" and binding.compute_dtype_of(None) == binding.MV_F32
    monkeypatch.setenv("MEMVUL_COMPUTE", "reference")
    assert binding.compute_dtype_of(None) == binding.MV_F32
    monkeypatch.delenv("MEMVUL_COMPUTE")
    assert binding.compute_dtype_of(None) == binding.MV_F16X8


def test_the_hook_is_bound():
    assert "mv_test_gemm_f32" in binding.ABI_SYMBOLS and hasattr(binding.Engine, "test_gemm_f32")


# ---- compare: every statistic by hand -----------------------------------------------------------------------------------------------------------------------------

def test_compare_statistics_by_hand():
    B, G = 10, 4
    ref = np.zeros((B, G, 2))
    ref[:, :, 0] = -1.0          # P(same) = sigmoid(-1) = 0.269 everywhere ...
    ref[3, 1, 0] = 1.0           # ... but row 3: anchor 1 at 0.731
    ref[5, 2, 0] = 0.002         # row 5: anchor 2 just above one half
    ref[7, 0, 0] = 0.5; ref[7, 3, 0] = 0.499  # row 7: anchors 0 and 3 nearly tied
    got = ref.copy()
    got[3, 1, 1] += 4e-4         # within tolerance
    got[5, 2, 0] -= 0.003        # over tolerance AND across the threshold (0.002 -> -0.001)
    got[7, 3, 0] += 0.002        # over tolerance AND the best anchor moves from 0 to 3
    r = audit.compare(ref, got, tol=1e-3, thres=0.5)
    d = np.abs(got - ref)
    assert r["rows"] == B and r["anchors"] == G
    assert r["max"] == pytest.approx(0.003) and not r["meets"]
    assert r["row_max"] == pytest.approx(d.reshape(B, -1).max(1).tolist())
    assert r["row_max_median"] == pytest.approx(0.0) and r["row_max_p90"] == pytest.approx(np.percentile(d.reshape(B, -1).max(1), 90))
    assert r["rms"] == pytest.approx(np.sqrt((4e-4 ** 2 + 0.003 ** 2 + 0.002 ** 2) / (B * G * 2)))
    assert r["p99"] == pytest.approx(np.percentile(d, 99)) and r["p999"] == pytest.approx(np.percentile(d, 99.9))
    assert r["rows_over"] == 2 and r["rows_over_idx"] == [5, 7]
    assert r["best_anchor_flips"] == 1 and r["threshold_crossings"] == 1
    json.dumps(r)  # plain Python numbers throughout
    ok = audit.compare(ref, ref + 1e-4)
    assert ok["meets"] and ok["rows_over"] == 0 and ok["best_anchor_flips"] == 0 and ok["threshold_crossings"] == 0
    assert audit.compare(ref, got, tol=5e-3)["meets"]
    # the other class as "same": the crossing is judged on that column
    assert audit.compare(ref, got, same_idx=1)["threshold_crossings"] in (0, 1)
    with pytest.raises(ValueError):
        audit.compare(ref, got[:, :3])


def test_sample_is_deterministic_and_covers_every_length_bucket():
    rng = np.random.default_rng(3)
    lens = np.concatenate([rng.integers(1, 65, 400), rng.integers(65, 129, 300), rng.integers(129, 257, 200), rng.integers(257, 513, 100)]).astype(np.int32)
    rng.shuffle(lens)
    rows = audit.sample_rows(lens, 64)
    assert np.array_equal(rows, audit.sample_rows(lens.copy(), 64)) and np.array_equal(rows, np.sort(rows)) and len(set(rows.tolist())) == len(rows) == 64
    buckets = lambda v: set(np.minimum((np.asarray(v) - 1) // 64, 7).tolist())  # noqa: E731
    assert buckets(lens[rows]) == buckets(lens)
    assert lens[rows].min() == lens.min() and lens[rows].max() == lens.max()  # both ends of the sorted input are taken
    assert np.array_equal(audit.sample_rows(lens, None), np.arange(len(lens))) and np.array_equal(audit.sample_rows(lens, 10 ** 6), np.arange(len(lens)))


# ---- audit over the oracle-backed stand-in ---------------------------------------------------------------------------------------------------------------------------

class _Standin(pu.OracleEngine):
    """The stand-in remembers the compute dtype it was loaded with; as "precise" it is off by a known 2e-3 in the rows holding PERTURBED ids."""
    created = []
    marks = ()

    def __init__(self, device=0, **kw):
        super().__init__(device, **kw)
        self.kw, self.closed = kw, False
        _Standin.created.append(self)

    def load_state_dict(self, sd, compute_dtype=1):
        super().load_state_dict(sd, compute_dtype)
        self.compute = compute_dtype

    def close(self):
        self.closed = True

    def forward_by_length(self, ids, lens, want_logits=True, want_probs=True, want_embed=False, min_tokens=None):
        out = self.forward(ids, lens)
        if self.compute == "precise":
            out["logits"] = out["logits"].copy()
            for b in range(ids.shape[0]):
                if int(ids[b, 1]) in _Standin.marks:
                    out["logits"][b, 0, 0] += 2e-3
        return out

    def attention_concentration(self):
        return (0.5, 3, 100) if self.compute == "precise" else (0.0, 0, 0)


@pytest.fixture(scope="module")
def small_case():
    from memvul_amd import synth
    dims = synth.BertDims(layers=2)
    w = synth.make_weights(dims, qk_scale=2.0, match_scale=6.0)
    ids, lens = synth.make_ids(12, 48, dims.vocab_size, seed=5, ragged=True, min_len=8)
    aids, alens = synth.make_ids(5, 70, dims.vocab_size, seed=6, ragged=True, min_len=10)
    return w, ids, lens, aids, alens


def test_audit_reports_the_perturbed_rows_and_only_those(small_case):
    w, ids, lens, aids, alens = small_case
    _Standin.created, _Standin.marks = [], (int(ids[2, 1]), int(ids[9, 1]))
    marked = [b for b in range(len(lens)) if int(ids[b, 1]) in _Standin.marks]
    res = audit.audit(w, ids, lens, aids, alens, forms=("precise", "safe"), engine_factory=_Standin)
    assert [e.compute for e in _Standin.created] == ["f32", "precise", "safe"] and all(e.closed for e in _Standin.created)
    assert all(e.kw["layers"] == 2 and e.kw["proj_dim"] == 512 for e in _Standin.created)
    assert res["rows"] == list(range(12)) and res["anchors"] == 5 and not res["meets"]
    p, s = res["forms"]["precise"], res["forms"]["safe"]
    assert not p["meets"] and p["rows_over"] == len(marked) and p["rows_over_idx"] == marked and p["max"] == pytest.approx(2e-3, rel=1e-3)
    assert p["monitors"] == {"max_collision": 0.5, "items_over": 3, "items_total": 100}
    assert s["meets"] and s["max"] == 0.0 and s["rows_over"] == 0
    assert res["reference"]["reports_per_s"] > 0 and p["reports_per_s"] > 0
    json.dumps(res)
    # a sample: the rows are named in the caller's numbering
    res2 = audit.audit(w, ids, lens, aids, alens, forms=("precise",), sample=6, engine_factory=_Standin)
    rows = audit.sample_rows(lens, 6).tolist()
    assert res2["rows"] == rows and res2["forms"]["precise"]["rows_over_idx"] == [b for b in marked if b in rows]
    with pytest.raises(ValueError):
        audit.audit(w, ids, lens, aids, alens, forms=("f32",), engine_factory=_Standin)


def test_the_anchors_run_at_their_own_padded_length(small_case):
    """Consecutive anchors of one padded length share a call; the bank keeps the file's order."""
    w, ids, lens, aids, alens = small_case
    calls = []

    class Rec(_Standin):
        def anchor_append(self, a, l):
            calls.append((a.shape, l.tolist()))
            super().anchor_append(a, l)

    _Standin.marks = ()
    audit.audit(w, ids[:2], lens[:2], aids, alens, forms=(), engine_factory=Rec)
    got = [n for _, ls in calls for n in ls]
    assert got == alens.tolist()
    for shape, ls in calls:
        assert len({audit._padded_len(n) for n in ls}) == 1 and shape[1] == max(ls)


def test_command_line_prints_one_json_line_and_its_status_says_meets(capsys, monkeypatch):
    root, arch, golden, test_path, w, dims = pu.make_fixture(n_irs=10, n_anchors=4, layers=2)
    try:
        monkeypatch.chdir(root)
        _Standin.created, _Standin.marks = [], ()
        rc = audit.main(["--archive", arch, "--golden", golden, "--input", test_path, "--forms", "precise,safe", "--sample", "8"], engine_factory=_Standin)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert rc == 0 and len(lines) == 1
        res = json.loads(lines[0])
        assert res["meets"] and set(res["forms"]) == {"precise", "safe"} and len(res["rows"]) == 8 and res["anchors"] == 4
        # a form that misses: every row carries the mark now
        _Standin.marks = tuple(range(dims.vocab_size))
        rc = audit.main(["--archive", arch, "--golden", golden, "--input", test_path], engine_factory=_Standin)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert rc == 1 and len(lines) == 1
        res = json.loads(lines[0])
        assert not res["meets"] and res["forms"]["precise"]["rows_over"] == 10 and "row_max" not in res["forms"]["precise"]
    finally:
        _Standin.marks = ()
        shutil.rmtree(root, ignore_errors=True)


# ---- the built kernel ---------------------------------------------------------------------------------------------------------------------------------------------

def _llvm_tool(name):
    cands = [shutil.which(name), os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc_path()))), "llvm", "bin", name),
             os.path.join(os.path.dirname(os.path.realpath(build.hipcc_path())), name)]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError(f"{name} of the ROCm installation not found next to hipcc")


def test_the_gemm_runs_on_the_fp32_matrix_instruction_without_scratch(tmp_path):
    """A VALU fallback must not pass as the feature: the three instantiations of gemm_f32_kernel in the built library hold the fp32-input MFMA, 64 of them per
    K-tile, and use no scratch memory; so does the attention kernel."""
    lib = build.build(verbose=False)
    (co,) = build.device_code_objects(lib)
    elf = tmp_path / "gfx950.co"
    elf.write_bytes(co)
    notes = subprocess.run([_llvm_tool("llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True, check=True).stdout
    kernels = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes):
        name = re.search(r"\.name:\s+(\S+)", blk)
        scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        if name and scratch:
            kernels[name.group(1)] = (int(scratch.group(1)), int(spill.group(1)) if spill else 0)
    gemms = sorted(k for k in kernels if "gemm_f32_kernel" in k)
    attn = [k for k in kernels if "attention_f32_kernel" in k]
    assert len(gemms) == 3 and len(attn) == 1, (gemms, attn)
    for k in gemms + attn:
        assert kernels[k] == (0, 0), (k, kernels[k])
        asm = subprocess.run([_llvm_tool("llvm-objdump"), "-d", f"--disassemble-symbols={k}", str(elf)], capture_output=True, text=True, check=True).stdout
        n = len(re.findall(r"v_mfma_f32_32x32x2_f32|v_mfma_f32_16x16x4_f32", asm))
        assert n >= 64, (k, n)
        assert "scratch_" not in asm
