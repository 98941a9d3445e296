"""Compute dtype "f32" (include/memvul_hip.h MV_F32): the reference form — the encoder in fp32 on the fp32-input MFMA (memvul_amd/csrc/ref_f32.h) — and the
contract audit built on it (memvul_amd/audit.py), on the GPU.

THE TOLERANCE.  The fp32 form is an fp32 implementation of the reference's arithmetic; what it may differ by is what two fp32 implementations differ by.  On
the 14 committed sink cases the committed fp32 reference (HF torch) reads 5.1 - 8.9e-6 against the float64 oracle (scripts/f32_form_make_refs.py prints it),
the numpy oracle in fp32 4.6 - 7.6e-6, the two against each other 6.6e-6 - 1.1e-5.  F32_TOL = 3e-5 = 3 x the largest of the first, rounded up: the margin
covers what the GPU does differently (one fmaf chain over K = 3072 where the CPU libraries sum in blocks, and a maximum over 96 logits that moves with any
re-ordering), and still sits a factor 2 under the smallest error any 16-bit form has read anywhere (7.4e-5), so an alias of another dtype cannot pass.
Every test records what it measured (gpu_util.record, names f32_form_*); a case that reads above F32_TOL is a finding to explain (order of summation? a
fast-math intrinsic in softmax / GELU / tanh?), not a bound to raise — as the GEMM test's bound was: one fmaf chain over K = 768 read 1.28 x it on the MI355X
(test_gemm_against_float64[2304-768-512], 'bias'), which is why ref_f32.h sums K in blocks of 32."""
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import audit, synth
from oracle import memvul_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

F32_TOL = 3e-5
LOGIT_TOL = 1e-3
SINK_CASES = (["sep_all_80_3001", "sep_all_95_3001", "sep_cls_80_3002", "cls_all_80_3001", "sep_all_50_3003"]
              + [f"{cell}_{seed}" for cell in ("mid_all_50", "mid_all_80", "mid_cls_80") for seed in (3001, 3002, 3003)])
L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0)
TRAINED = dict(qk_scale=2.0, match_scale=29.0, trained_like=True)


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def sink_refs(golden_dir):
    return np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))


@pytest.fixture(scope="module")
def refs64(golden_dir):
    return np.load(os.path.join(golden_dir, "f32_form_refs.npz"))


def _engine(dims, w, compute, **kw):
    from memvul_amd.binding import Engine

    opts = dict(max_tokens=16 * 512, max_batch=16, max_anchors=16)
    opts.update(kw)
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, **opts)
    eng.load_state_dict(w, compute)
    return eng


def _sink_logits(refs, case, compute):
    """The logits of one sink case in one compute dtype, fed as tests/test_safe_form_gpu.py::_sink_logits_err feeds it: one anchor per call, each at the padded
    length of its own token count, the 8 issue reports as one batch of 256 tokens."""
    import test_safe_form_gpu as tsf

    dims, w, ids, lens, aids, alens = tsf._sink_case(refs, case)
    eng = _engine(dims, w, compute)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for g in range(len(alens)):
                eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
            return eng.forward(ids, lens)["logits"]
    finally:
        eng.close()


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SINK_CASES)
def test_sink_cases_against_float64_and_the_committed_reference(gu, sink_refs, refs64, case):
    lg = _sink_logits(sink_refs, case, "f32")
    e64 = float(np.abs(lg.astype(np.float64) - refs64[case]).max())
    e32 = float(np.abs(lg - sink_refs[case + "_lg"]).max())
    print(f"f32 form {case}: against float64 {e64:.3e}, against the committed fp32 reference {e32:.3e}")
    gu.record("f32_form_sink", case=case, err_float64=e64, err_committed_fp32=e32, logit_scale=float(np.abs(refs64[case]).max()))
    assert e64 <= F32_TOL, e64
    assert e32 <= F32_TOL, e32


def test_diffuse_draws_against_the_committed_reference(gu, golden_dir):
    """The 24 seed_* draws of tests/golden/r05_trained_like_refs.npz (8 issue reports x 256 tokens against 6 anchors of up to 512, anchors as one chunk padded
    to its longest, as the reference ran them)."""
    import r05_make_refs as mk

    refs = np.load(os.path.join(golden_dir, "r05_trained_like_refs.npz"))
    errs = {}
    for seed in mk.SEEDS:
        dims, ids, lens, aids, alens = mk.case_inputs(seed)
        w = synth.make_weights(dims, seed=seed, **TRAINED)
        eng = _engine(dims, w, "f32")
        try:
            LA = int(alens.max())
            eng.anchor_append(aids[:, :LA], alens)
            errs[seed] = float(np.abs(eng.forward(ids, lens)["logits"] - refs[f"seed_{seed}"]).max())
        finally:
            eng.close()
    print("f32 form, diffuse draws:", errs)
    gu.record("f32_form_diffuse", **{f"seed_{s}": e for s, e in errs.items()})
    assert all(e <= F32_TOL for e in errs.values()), errs


def test_length_draws_against_the_committed_reference(gu, golden_dir):
    """The len_* draws, compared the way tests/test_safe_form_gpu.py compares them (embeddings turned into logits against outlier_1_u): every padded length
    the planner produces."""
    import r05_make_refs as mk

    refs = np.load(os.path.join(golden_dir, "r05_trained_like_refs.npz"))
    dk, wk = dict(layers=12), dict(seed=mk.ENV_SEED, **TRAINED)
    dims, w = gu.weights_for(dk, wk)
    eng = gu.engine_for(dk, wk, compute_dtype="f32")
    u_ref = refs["outlier_1_u"]
    errs = {}
    for L in mk.LENGTHS:
        _, ids, lens = mk.length_inputs(L)
        v = eng.encode(ids, lens)
        lg_g = orc.match(u_ref, v, w[synth.KEY_MATCH_W])[0]
        lg_r = orc.match(u_ref, refs[f"len_{L}"], w[synth.KEY_MATCH_W])[0]
        errs[L] = float(np.abs(lg_g - lg_r).max())
    print("f32 form, length draws:", errs)
    gu.record("f32_form_length_draws", **{f"len_{L}": e for L, e in errs.items()})
    assert all(e <= F32_TOL for e in errs.values()), errs


@pytest.mark.parametrize("name", ["l12_trained_s256", "l12_trained_ragged", "l12_base_ragged", "l12_base_s256", "l2_peaky_full", "l2_ragged"])
def test_goldens(gu, golden_dir, name):
    import make_golden

    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    dk, wk, B, S, ragged, G, SA = make_golden.CASES[name]
    eng = gu.engine_for(dk, wk, compute_dtype="f32", max_tokens=16384, max_batch=64, max_anchors=64)
    eng.anchor_reset()
    LA = int(g["anchor_lens"].max())
    eng.anchor_append(g["anchor_ids"][:, :LA], g["anchor_lens"])
    out = eng.forward(g["ids"], g["lens"], want_embed=True)
    errs = dict(logits=float(np.abs(out["logits"] - g["logits"]).max()), p=float(np.abs(out["probs"] - g["p"]).max()),
                u=float(np.abs(out["embed"] - g["u"]).max()), logit_scale=float(np.abs(g["logits"]).max()))
    print(f"f32 form {name}:", errs)
    gu.record("f32_form_golden", case=name, **errs)
    eng.anchor_reset()
    assert errs["logits"] <= F32_TOL, errs
    assert np.array_equal(out["best_idx"], g["idx"].astype(np.int32)) or errs["p"] <= F32_TOL


def test_ref12_the_references_own_run(gu):
    """tests/golden/ref12: the reference's own code executed.  Logits at F32_TOL; anchor bank and probabilities at 3 x the 5e-6 tests/test_reference_pin.py
    uses for oracle-vs-reference."""
    import test_reference_pin as trp

    ref = trp.get_ref("ref12")
    aids, amask = trp._pad(ref["reader"]["golden"])
    ids, mask = trp._pad(ref["reader"]["test"])
    dk = dict(layers=ref["meta"]["layers"], vocab_size=ref["meta"]["vocab_size"])
    wk = dict(ref["meta"]["weight_kwargs"])
    eng = gu.engine_for(dk, wk, compute_dtype="f32", max_tokens=32 * 512, max_batch=32, max_anchors=16)
    eng.anchor_reset()
    eng.anchor_append(aids.astype(np.int32), amask.sum(1).astype(np.int32))
    v = eng.anchor_get()
    out = eng.forward(ids.astype(np.int32), mask.sum(1).astype(np.int32))
    errs = dict(v=float(np.abs(v - ref["anchors"]).max()), logits=float(np.abs(out["logits"] - ref["logits"]).max()),
                p=float(np.abs(out["probs"] - ref["probs"]).max()))
    print("f32 form ref12:", errs)
    gu.record("f32_form_ref12", **errs)
    eng.anchor_reset()
    assert errs["logits"] <= F32_TOL and errs["v"] <= 1.5e-5 and errs["p"] <= 1.5e-5, errs


# ---- 2. the GEMM alone --------------------------------------------------------------------------------------------------------------------------------------------

def _gelu64(x):
    from math import erf
    return x * 0.5 * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


@pytest.mark.parametrize("M", [512, 4096])
@pytest.mark.parametrize("N,K", [(2304, 768), (768, 768), (3072, 768), (768, 3072)])
def test_gemm_against_float64(gu, M, N, K):
    """|C - C64| <= 2 g(K) (|A| |W|^T + |bias| + |res|) elementwise, g = 1.5e-7 for K = 768 and 3.5e-7 for K = 3072 (the fmaf chain's measured constants);
    GELU / residual epilogues compared after the same float64 epilogue (GELU is 1-Lipschitz up to 1.13: the bound on its argument, x 1.13, + 4 fp32 roundings
    of the result)."""
    import f32_stage_kit as fsk  # (the bound lives there: tests/test_f32_stage_gpu.py holds the engine's own launches to it)

    eng = gu.engine_for(L2, WK, compute_dtype="f32")
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    g = fsk.gemm_g(K)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    pre = A64 @ W64.T + bias
    mag = np.abs(A64) @ np.abs(W64).T + np.abs(bias)
    worst = {}
    for act in ("bias", "gelu", "res"):
        C, ms = eng.test_gemm_f32(A, W, bias, res if act == "res" else None, act=act)
        if act == "bias":
            want, bound = pre, fsk.gemm_bound("bias", g, mag)
        elif act == "gelu":
            want = _gelu64(pre[:64])  # (the float64 erf is a Python loop: 64 rows of it)
            C, bound = C[:64], fsk.gemm_bound("gelu", g, mag[:64], want=want)
        else:
            want, bound = pre + res, fsk.gemm_bound("res", g, mag, res=res)
        worst[act] = float((np.abs(C - want) / bound).max())
        assert np.all(np.abs(C - want) <= bound), (act, worst)
    gu.record("f32_form_gemm", M=M, N=N, K=K, **{f"err_over_bound_{a}": v for a, v in worst.items()})


def test_gemm_rejects_shapes_it_does_not_tile(gu):
    eng = gu.engine_for(L2, WK, compute_dtype="f32")
    with pytest.raises(RuntimeError):
        eng.test_gemm_f32(np.zeros((100, 64), np.float32), np.zeros((128, 64), np.float32), None)
    with pytest.raises(RuntimeError):
        eng.test_gemm_f32(np.zeros((128, 64), np.float32), np.zeros((128, 64), np.float32), None, None, act="res")


# ---- 3. a row's bits and the batch it travels in ------------------------------------------------------------------------------------------------------------------

def test_row_bits_do_not_depend_on_the_batch(gu):
    dk, wk = dict(layers=3, vocab_size=2048), dict(qk_scale=2.0, match_scale=6.0)
    dims, w = gu.weights_for(dk, wk)
    eng = gu.engine_for(dk, wk, compute_dtype="f32", max_tokens=64 * 256, max_batch=64, max_anchors=32)
    ids, lens = synth.make_ids(64, 200, dims.vocab_size, ragged=True, min_len=5)
    aids, alens = synth.make_ids(9, 96, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=5)
    # anchors appended in chunks of 1 / 5 / all
    banks = []
    for chunk in (1, 5, 9):
        eng.anchor_reset()
        for g0 in range(0, 9, chunk):
            eng.anchor_append(aids[g0:g0 + chunk], alens[g0:g0 + chunk])
        banks.append(eng.anchor_get())
    assert np.array_equal(banks[0], banks[1]) and np.array_equal(banks[0], banks[2])
    out = eng.forward(ids, lens, want_embed=True)
    # a permuted batch
    perm = np.random.default_rng(1).permutation(64)
    o2 = eng.forward(ids[perm], lens[perm], want_embed=True)
    assert np.array_equal(o2["embed"], out["embed"][perm]) and np.array_equal(o2["logits"], out["logits"][perm])
    # a row alone against the same row among 63 others
    for r in (0, 17, 63):
        o1 = eng.forward(ids[r:r + 1], lens[r:r + 1], want_embed=True)
        assert np.array_equal(o1["embed"][0], out["embed"][r]) and np.array_equal(o1["logits"][0], out["logits"][r])
    # padding columns added (200 -> 256: the same padded length)
    wide = np.zeros((64, 256), np.int32)
    wide[:, :200] = ids
    assert np.array_equal(eng.forward(wide, lens)["logits"], out["logits"])
    # the resident-corpus path against mv_forward at the same width, two streams against one
    eng.corpus_upload(ids, lens)
    eng.corpus_run(0, 64, 16, keep_probs=True)
    best, idx, ps = eng.corpus_results(0, 64, with_probs=True)
    assert np.array_equal(ps, out["probs"][:, :, 0]) and np.array_equal(idx, out["best_idx"]) and np.array_equal(best, out["best"])
    eng.set_streams(1)
    eng.corpus_run(0, 64, 16, keep_probs=True)
    best1, idx1, ps1 = eng.corpus_results(0, 64, with_probs=True)
    eng.set_streams(2)
    assert np.array_equal(ps1, ps) and np.array_equal(idx1, idx) and np.array_equal(best1, best)
    # forward_by_length and its two halves
    a = eng.forward_by_length(ids, lens, min_tokens=2048)
    t = eng.forward_by_length_begin(ids, lens, min_tokens=2048)
    assert t[0] == "pending"
    b = eng.forward_by_length_end(t)
    assert all(np.array_equal(a[k], b[k]) for k in ("logits", "probs", "best", "best_idx"))
    longest = lens > 192  # these ran at the batch's own padded length in both forms
    assert longest.any() and np.array_equal(a["logits"][longest], out["logits"][longest])
    assert float(np.abs(a["logits"] - out["logits"]).max()) <= F32_TOL  # another padded length: the same arithmetic on the unmasked keys
    eng.anchor_reset()


# ---- 4. every entry point answers -----------------------------------------------------------------------------------------------------------------------------------

def test_entry_points_forms_monitors_and_taps(gu):
    from memvul_amd.binding import Engine

    dk, wk = dict(layers=12), dict()
    dims, w = gu.weights_for(dk, wk)
    eng = gu.engine_for(dk, wk, compute_dtype="f32", max_tokens=8192, max_batch=64, max_anchors=32)
    ids, lens = synth.make_ids(3, 70, dims.vocab_size, ragged=True, min_len=20)
    mask = synth.mask_from_lens(lens, 70)
    taps = {}
    u64 = orc.instance_forward(w, ids.astype(np.int64), mask, dtype=np.float64, taps=taps)
    # debug taps 0 and 10 against the float64 oracle after 0, 1 and 12 layers: 3e-5 x the state's own scale (the logit bound, carried to a tensor of that size)
    for n_layers, key in ((0, "embed"), (1, "layer0"), (12, "layer11")):
        eng.debug_encode(ids, lens, n_layers)
        hid = eng.debug_read(0)[:, :70]
        scale = max(1.0, float(np.abs(taps[key]).max()))
        e = float(np.abs(hid - taps[key])[mask].max())
        gu.record("f32_form_tap", n_layers=n_layers, err=e, scale=scale)
        assert e <= F32_TOL * scale, (n_layers, e, scale)
    assert float(np.abs(eng.debug_read(10) - u64).max()) <= F32_TOL
    for tap in (1, 5, 9):
        with pytest.raises(RuntimeError, match="fp16"):
            eng.debug_read(tap)
    # forms and monitors
    with pytest.raises(RuntimeError):
        eng.set_form("safe")
    with pytest.raises(RuntimeError):
        eng.set_form("guarded")
    assert eng.form == "default"
    # encode / forward / match / topk / bucketed_sweep agree with each other and with the oracle
    aids, alens = synth.make_ids(8, 64, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=8)
    eng.anchor_reset()
    eng.anchor_append(aids, alens)
    v = eng.anchor_get()
    u = eng.encode(ids, lens)
    assert float(np.abs(u - u64).max()) <= F32_TOL
    out = eng.forward(ids, lens, want_embed=True)
    assert np.array_equal(out["embed"], u)
    assert np.array_equal(eng.match(u)["logits"], out["logits"])
    tp, ti = eng.topk(u, 3)
    assert np.array_equal(ti[:, 0], out["best_idx"]) and np.array_equal(tp[:, 0], out["best"][:, 0])
    best, idx, ps = eng.bucketed_sweep(ids, lens, 2, with_probs=True)
    assert np.array_equal(idx, out["best_idx"]) and float(np.abs(ps - out["probs"][:, :, 0]).max()) <= F32_TOL
    lg64 = orc.match(u64, v.astype(np.float64), w[synth.KEY_MATCH_W])[0]
    assert float(np.abs(out["logits"] - lg64).max()) <= F32_TOL
    assert eng.x8_saturation() == 0 and eng.attention_concentration() == (0.0, 0, 0)
    # S in {1, 7, 64, 65, 300, 512} with B = 1 and B = 33: finite, and the first row equals the row alone
    for S in (1, 7, 64, 65, 300, 512):
        i33, l33 = synth.make_ids(33, S, dims.vocab_size, seed=S, ragged=S > 7, min_len=min(S, 3))
        e = gu.engine_for(dk, wk, compute_dtype="f32", max_tokens=33 * 512, max_batch=64, max_anchors=32)
        if e.n_anchors == 0:
            e.anchor_append(aids, alens)
        o33 = e.forward(i33, l33)
        o1 = e.forward(i33[:1], l33[:1])
        assert np.isfinite(o33["logits"]).all() and np.array_equal(o33["logits"][0], o1["logits"][0]), S
    # over capacity
    small = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=1024, max_batch=8, max_anchors=8)
    try:
        small.load_state_dict(w, "f32")
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            small.debug_encode(np.ones((8, 256), np.int32), np.full(8, 256, np.int32), 1)
        small.anchor_append(aids[:2], alens[:2])
        assert np.isfinite(small.forward(np.ones((8, 256), np.int32), np.full(8, 256, np.int32))["logits"]).all()  # walked in passes, like the other dtypes
    finally:
        small.close()
    eng.anchor_reset()


def test_memvul_form_with_the_reference_form_fails(gu, monkeypatch):
    from memvul_amd.binding import Engine

    dims, w = gu.weights_for(L2, WK)
    monkeypatch.setenv("MEMVUL_FORM", "safe")
    eng = Engine(0, vocab_size=dims.vocab_size, layers=2, max_tokens=1024, max_batch=8, max_anchors=8)
    try:
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            eng.load_state_dict(w, "f32")
    finally:
        eng.close()


# ---- 5. the other dtypes are untouched ------------------------------------------------------------------------------------------------------------------------------

def test_precise_and_f16_bits_before_and_after_an_f32_engine(golden_dir):
    import make_golden

    name = "l12_trained_s256"
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    dk, wk, B, S, ragged, G, SA = make_golden.CASES[name]
    dims = synth.BertDims(**dk)
    w = synth.make_weights(dims, **wk)
    LA = int(g["anchor_lens"].max())

    def logits(compute):
        eng = _engine(dims, w, compute, max_tokens=16384, max_batch=64, max_anchors=64)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                eng.anchor_append(g["anchor_ids"][:, :LA], g["anchor_lens"])
                return eng.forward(g["ids"], g["lens"])["logits"]
        finally:
            eng.close()

    before = {c: logits(c) for c in ("precise", "f16")}
    f32 = logits("f32")
    after = {c: logits(c) for c in ("precise", "f16")}
    for c in ("precise", "f16"):
        assert before[c].tobytes() == after[c].tobytes(), c
        assert not np.array_equal(before[c], f32)
    assert float(np.abs(f32 - g["logits"]).max()) <= F32_TOL


# ---- 6. the audit, end to end ----------------------------------------------------------------------------------------------------------------------------------------

def test_audit_on_an_ordinary_token_sink_and_on_a_diffuse_draw(gu, sink_refs):
    import r05_make_refs as mk
    import test_safe_form_gpu as tsf

    case = "mid_all_80_3001"
    dims, w, ids, lens, aids, alens = tsf._sink_case(sink_refs, case)
    opts = dict(max_tokens=16 * 512, max_batch=16, max_anchors=16)
    res = audit.audit(w, ids, lens, aids, alens, forms=("precise", "safe"), engine_options=opts, keep_logits=True)
    by_hand = {c: _sink_logits(sink_refs, c2, c) for c, c2 in (("f32", case), ("precise", case), ("safe", case))}
    rec = {}
    for f in ("precise", "safe"):
        r = res["forms"][f]
        hand = float(np.abs(by_hand[f].astype(np.float64) - by_hand["f32"]).max())
        committed = float(np.abs(by_hand[f] - sink_refs[case + "_lg"]).max())  # what _sink_logits_err reports
        rec[f] = dict(audit=r["max"], by_hand=hand, against_committed=committed, monitors=r["monitors"], reports_per_s=r["reports_per_s"])
        assert r["max"] == hand, (f, r["max"], hand)
        assert abs(r["max"] - committed) <= F32_TOL, (f, r["max"], committed)
    print("audit", case, rec)
    gu.record("f32_form_audit", case=case, **{f"{f}_{k}": v for f, d in rec.items() for k, v in d.items() if k != "monitors"},
              precise_items_over=res["forms"]["precise"]["monitors"]["items_over"], reference_reports_per_s=res["reference"]["reports_per_s"])
    p, s = res["forms"]["precise"], res["forms"]["safe"]
    assert not p["meets"] and p["max"] > LOGIT_TOL and p["rows_over"] >= 1 and p["monitors"]["items_over"] > 0
    assert s["meets"] and s["max"] <= LOGIT_TOL
    assert not res["meets"]
    # a diffuse draw: both meet
    dims, ids, lens, aids, alens = mk.case_inputs(3001)
    w = synth.make_weights(dims, seed=3001, **TRAINED)
    res = audit.audit(w, ids, lens, aids, alens, forms=("precise", "safe"), engine_options=opts)
    gu.record("f32_form_audit", case="seed_3001", precise=res["forms"]["precise"]["max"], safe=res["forms"]["safe"]["max"])
    assert res["meets"] and res["forms"]["precise"]["meets"] and res["forms"]["safe"]["meets"]
