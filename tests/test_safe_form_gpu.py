"""The SAFE form of compute dtype MV_F16X8 (include/memvul_hip.h mv_set_form; binding compute dtype name "safe"), on the GPU.

The default form holds the 1e-3 logit contract for diffuse attention and for attention sinks on [CLS] / [SEP]; with most of a head's mass on an ORDINARY token it
reads 0.8 - 2.7e-3 (profiles/r06_n_sink_envelope.txt).  The safe form sweeps both first-order correction terms in every row of every GEMM, the A-side term in all
three QKV blocks, and carries Q, K, V, P as hi + lo fp16 planes through attention at every padded length (attention_v2.h VLO with NCH > 1 above 128 keys) and
through the pruned last layer's single-query attention.  oracle/precision_model.py prices it at 9.5e-5 on mid_all_80_3001 (tests/test_safe_form_cpu.py)."""
import os
import sys
import warnings

import numpy as np
import pytest

from memvul_amd import synth
from oracle import memvul_oracle as orc

from stage_kit import attention64 as _attention64  # (shared with tests/test_stage_parity_gpu.py)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LOGIT_TOL = 1e-3  # the project's contract (tests/test_gpu_parity.py LOGIT_TOL)
L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0)  # the peaked 2-layer model of tests/test_gpu_kernels.py


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def sink_refs(golden_dir):
    return np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))


_cases = {}


def _sink_case(refs, case):
    """(dims, weights, ids, lens, aids, alens) of a committed sink case, rebuilt from its stored gains (scripts/r06_make_sink_refs.py)."""
    import r06_make_sink_refs as mk6

    if case not in _cases:
        if len(_cases) >= 2:
            _cases.pop(next(iter(_cases)))
        token, rows, pct, seed = case.split("_")
        _cases[case] = mk6.case(token, rows, int(pct) / 100.0, int(seed), gains=refs[case + "_gains"])[:6]
    return _cases[case]


def _sink_engine(dims, w, compute):
    from memvul_amd.binding import Engine

    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=16 * 512, max_batch=16, max_anchors=16)
    eng.load_state_dict(w, compute)
    return eng


def _sink_logits_err(refs, case, compute):
    """max |logits - CPU reference| of one sink case in one form: 8 issue reports x 256 tokens against 6 anchors of up to 512 tokens (the anchors' passes run
    at their own padded lengths up to 512: every chunked two-plane instantiation is on the path)."""
    dims, w, ids, lens, aids, alens = _sink_case(refs, case)
    eng = _sink_engine(dims, w, compute)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the default form warns about the sink: that is the other tests' subject)
            for g in range(len(alens)):  # one anchor per call: each runs at the padded length of its own token count
                eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
            out = eng.forward(ids, lens)
        return float(np.abs(out["logits"] - refs[case + "_lg"]).max()), eng.x8_saturation(), eng.form
    finally:
        eng.close()


MID_CELLS = ("mid_all_50", "mid_all_80", "mid_cls_80")


@pytest.mark.parametrize("seed", [3001, 3002, 3003])
@pytest.mark.parametrize("cell", MID_CELLS)
def test_safe_form_holds_the_contract_on_ordinary_token_sinks(gu, sink_refs, cell, seed):
    """1. The contract where no form of the library held it: 50 / 80 % of every row's (or the [CLS] row's) attention mass on one ordinary token."""
    case = f"{cell}_{seed}"
    e, sat, form = _sink_logits_err(sink_refs, case, "safe")
    print(f"safe form {case}: max |logit error| {e:.3e}")
    gu.record("safe_form_sink", case=case, logits_err=e, logit_scale=float(np.abs(sink_refs[case + "_lg"]).max()), mass=float(sink_refs[case + "_stat"][0]),
              eff_keys=float(sink_refs[case + "_stat"][1]), x8_saturation=sat)
    assert form == "safe"
    assert e <= LOGIT_TOL, e
    assert sat == 0


@pytest.mark.parametrize("cell", MID_CELLS)
def test_saturated_calibrations_are_run_and_recorded(gu, sink_refs, cell):
    """Seed 3004 of each cell is a saturated calibration (mass 1.00, ONE effective key; the default form reads 3e-2 on one of them): run and recorded in both
    forms, no bound asserted (DESIGN.md section 2 says what they read)."""
    case = f"{cell}_3004"
    e_safe, sat, _ = _sink_logits_err(sink_refs, case, "safe")
    e_def, _, _ = _sink_logits_err(sink_refs, case, "precise")
    print(f"saturated {case}: safe {e_safe:.3e} default {e_def:.3e}")
    gu.record("safe_form_saturated_sink", case=case, logits_err_safe=e_safe, logits_err_default=e_def, mass=float(sink_refs[case + "_stat"][0]),
              eff_keys=float(sink_refs[case + "_stat"][1]), x8_saturation=sat)
    assert np.isfinite(e_safe) and np.isfinite(e_def)


def test_the_sink_test_tells_the_forms_apart(gu, sink_refs):
    """2. An alias of the default form must not pass as "safe": on mid_all_80_3001 the default form reads above the contract (2.1e-3 measured, profiles/) and
    more than twice the safe form."""
    e_def, _, form_def = _sink_logits_err(sink_refs, "mid_all_80_3001", "precise")
    e_safe, _, form_safe = _sink_logits_err(sink_refs, "mid_all_80_3001", "safe")
    print(f"mid_all_80_3001: default {e_def:.3e} safe {e_safe:.3e}")
    gu.record("safe_vs_default_form", case="mid_all_80_3001", err_default=e_def, err_safe=e_safe)
    assert (form_def, form_safe) == ("default", "safe")
    assert e_def > 2 * e_safe, (e_def, e_safe)


@pytest.mark.parametrize("case", ["sep_all_80_3001", "sep_all_95_3001", "sep_cls_80_3002", "cls_all_80_3001", "sep_all_50_3003"])
def test_safe_form_on_the_delimiter_sinks(gu, sink_refs, case):
    """3. No regression where the default already holds: the five delimiter-sink cases of tests/test_gpu_parity.py."""
    e, sat, _ = _sink_logits_err(sink_refs, case, "safe")
    print(f"safe form {case}: {e:.3e}")
    gu.record("safe_form_delimiter_sink", case=case, logits_err=e, x8_saturation=sat)
    assert e <= LOGIT_TOL and sat == 0, (e, sat)


def test_safe_form_on_the_trained_like_length_draws(gu, golden_dir):
    """3. ... and the draws of tests/golden/r05_trained_like_refs.npz the precise-mode test of the short passes uses (16 sequences of 8 / 16 / 32 / 64 tokens
    on the envelope model; logit error = what the embedding's error costs against 8 fixed issue-report embeddings), plus the longer draws of the same file."""
    import r05_make_refs as mk

    refs = np.load(os.path.join(golden_dir, "r05_trained_like_refs.npz"))
    dk, wk = dict(layers=12), dict(seed=mk.ENV_SEED, qk_scale=2.0, match_scale=29.0, trained_like=True)
    dims, w = gu.weights_for(dk, wk)
    eng = gu.engine_for(dk, wk, compute_dtype="safe")
    assert eng.form == "safe"
    u_ref = refs["outlier_1_u"]
    errs = {}
    for L in (8, 16, 32, 64, 128, 192, 256, 384, 512):
        _, ids, lens = mk.length_inputs(L)
        v = eng.encode(ids, lens)
        lg_g = orc.match(u_ref, v, w[synth.KEY_MATCH_W])[0]
        lg_r = orc.match(u_ref, refs[f"len_{L}"], w[synth.KEY_MATCH_W])[0]
        errs[L] = float(np.abs(lg_g - lg_r).max())
    print("safe form, length draws:", errs)
    gu.record("safe_form_length_draws", **{f"len_{L}": e for L, e in errs.items()})
    assert all(e <= LOGIT_TOL for e in errs.values()), errs
    assert eng.x8_saturation() == 0


# ---- 4. the kernel alone ---------------------------------------------------------------------------------------------------------------------------------------

def _taps(gu, B, S, ragged):
    dims, w = gu.weights_for(L2, WK)
    ids, lens = synth.make_ids(B, S, dims.vocab_size, ragged=ragged)
    taps = {}
    mask = synth.mask_from_lens(lens, S)
    orc.instance_forward(w, ids.astype(np.int64), mask, taps=taps)
    return ids, lens, mask, taps


@pytest.mark.parametrize("B,S,ragged", [(2, 64, False), (3, 128, True), (2, 192, True), (2, 256, True), (1, 320, True), (2, 100, True), (2, 384, True),
                                        (2, 512, True), (1, 500, True)])
def test_layer0_context_in_the_safe_form(gu, B, S, ragged):
    """4a. The shapes of test_gpu_kernels.test_layer0_stages, engine in the safe form: layer-0 context against the oracle tap within that test's bound for the
    precise dtype — the chunked two-plane path computes attention (masks, chunk hand-over, rescale)."""
    ids, lens, mask, taps = _taps(gu, B, S, ragged)
    eng = gu.engine_for(L2, WK, compute_dtype="safe")
    eng.debug_encode(ids, lens, 1)
    ctx = eng.debug_read(5)[:, :S].astype(np.float32)
    err = float(np.abs(ctx - taps["l0_ctx"])[mask].max())
    gu.record("safe_form_layer0_ctx", B=B, S=S, max_err=err)
    assert err < 6e-3, err


@pytest.mark.parametrize("B,S", [(48, 256), (70, 128), (40, 192), (26, 512), (30, 384), (21, 320)])
def test_attention_item_loop_in_the_safe_form(gu, B, S):
    """4a. The shapes of test_gpu_kernels.test_attention_persistent_item_loop: more units than resident workgroups (one per CU for the 128 KiB rings), uneven
    tails, ragged lengths, two to four key chunks per unit."""
    ids, lens, mask, taps = _taps(gu, B, S, True)
    Sp = (S + 63) // 64 * 64 if S <= 256 else (S + 127) // 128 * 128
    eng = gu.engine_for(L2, WK, compute_dtype="safe", max_tokens=B * Sp, max_batch=B)
    eng.debug_encode(ids, lens, 1)
    ctx = eng.debug_read(5)[:, :S].astype(np.float32)
    err = float(np.abs(ctx - taps["l0_ctx"])[mask].max())
    gu.record("safe_form_attention_items", B=B, S=S, max_err=err)
    assert err < 8e-3, err


@pytest.mark.parametrize("S", [128, 192, 256, 384, 512])
def test_two_plane_attention_on_the_engines_own_operands(gu, S):
    """4b. Sharper than 4a: the engine's own Q, K, V^T planes (debug buffers 2 - 4 and their low planes 7 - 9) through float64 attention, against the context the
    kernel wrote (5).  S = 128 is the two-plane instantiation the default form ships (the control), 192 .. 512 are the chunked ones.
      (i)  |ctx - ctx64_two| <= 2^-11 |ctx64_two| + 2^-14 max|V| (per head) — the fp16 rounding of the stored context; fp32 accumulation over at most 512
           products (512 x 2^-24 = 2^-15), the fp32 exponent argument and the dropped lo x lo terms (2^-22), with a factor 2.  Derived, not measured.
      (ii) rms(ctx - ctx64_two) < rms(ctx - ctx64_one): the kernel is closer to the two-plane arithmetic than to the one-plane arithmetic (hi planes, P rounded
           to fp16).  The model is peaked (qk_scale = 4), so the two differ above the output rounding.
    And: hi + lo of the planes is closer to the oracle's fp32 Q / K / V than hi alone, by 4x at least (11 against 22 bits; the GEMM's own error is the floor)."""
    B = 2
    ids, lens, mask, taps = _taps(gu, B, S, True)
    eng = gu.engine_for(L2, WK, compute_dtype="safe")
    eng.debug_encode(ids, lens, 1)
    f64 = lambda b: eng.debug_read(b).astype(np.float64)
    qh, kh, vh = f64(2)[:, :, :S], f64(3)[:, :, :S], f64(4)[:, :, :, :S].transpose(0, 1, 3, 2)
    ql, kl, vl = f64(7)[:, :, :S], f64(8)[:, :, :S], f64(9)[:, :, :, :S].transpose(0, 1, 3, 2)
    ctx = f64(5)[:, :S].reshape(B, S, 12, 64).transpose(0, 2, 1, 3)  # [B, 12, S, 64]
    two = _attention64(qh + ql, kh + kl, vh + vl, lens, round_p=False)
    one = _attention64(qh, kh, vh, lens, round_p=True)
    m = np.broadcast_to(mask[:, None, :, None], ctx.shape)
    vmax = np.abs(np.where(m, vh + vl, 0.0)).max(axis=(2, 3), keepdims=True)
    bound = 2.0 ** -11 * np.abs(two) + 2.0 ** -14 * vmax
    d_two, d_one = (ctx - two)[m], (ctx - one)[m]
    worst = float((np.abs(ctx - two) / bound)[m].max())
    rms_two, rms_one = float(np.sqrt((d_two ** 2).mean())), float(np.sqrt((d_one ** 2).mean()))
    # the low planes against the oracle's fp32 taps
    gain = {}
    for name, hi, lo, tap in (("q", qh * 8.0, ql * 8.0, taps["l0_q"]), ("k", kh, kl, taps["l0_k"]), ("v", vh, vl, taps["l0_v"])):
        e_hi, e_two = float(np.abs(hi - tap)[m].max()), float(np.abs(hi + lo - tap)[m].max())
        gain[name] = (e_hi, e_two)
    print(f"S {S}: max |ctx - two| / bound {worst:.3f}  rms two {rms_two:.3e} one {rms_one:.3e}  planes {gain}")
    gu.record("safe_form_two_plane_kernel", S=S, max_err_over_bound=worst, max_abs_err=float(np.abs(d_two).max()), rms_vs_two_plane=rms_two, rms_vs_one_plane=rms_one,
              **{f"{n}_err_hi": e[0] for n, e in gain.items()}, **{f"{n}_err_hi_lo": e[1] for n, e in gain.items()})
    assert worst <= 1.0, worst
    assert rms_two < rms_one, (rms_two, rms_one)
    for name, (e_hi, e_two) in gain.items():
        assert e_two * 4 <= e_hi, (name, e_hi, e_two)


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------------------------------------------

def test_a_rows_bits_do_not_depend_on_its_batch_in_the_safe_form(gu):
    """5. A row's embedding bits are the same alone, in a permuted batch of its padded length, through forward_by_length and its two halves, and (as P(same)
    against the bank) through the resident sweep with 1 and 2 streams — padded lengths 64 .. 512.  MEMVUL_CLS_ASIDE / MEMVUL_QKV_ASIDE do not reach the form."""
    dk, wk = dict(layers=3, vocab_size=2048), dict(qk_scale=2.0, match_scale=6.0)
    dims, w = gu.weights_for(dk, wk)
    per = 6
    want = np.repeat(np.array([40, 64, 100, 128, 150, 192, 230, 256, 300, 384, 450, 512], np.int32), per // 2)  # 6 rows per padded length, 36 rows
    ids, _ = synth.make_ids(len(want), 512, dims.vocab_size, ragged=False)
    lens = want.copy()
    ids = (ids * (np.arange(512)[None, :] < lens[:, None])).astype(np.int32)
    order = np.random.default_rng(7).permutation(len(lens))
    ids, lens = np.ascontiguousarray(ids[order]), lens[order]
    B = len(lens)
    kw = dict(max_tokens=B * 512, max_batch=64, max_anchors=32)
    eng = gu.engine_for(dk, wk, compute_dtype="safe", **kw)
    assert eng.form == "safe"
    eng.anchor_reset()
    eng.anchor_set(synth.make_anchor_bank(24))
    alone = np.empty((B, 512), np.float32)
    p_alone = np.empty((B, 24), np.float32)
    for i in range(B):
        o = eng.forward(ids[i:i + 1, :int(lens[i])], lens[i:i + 1], want_embed=True)
        alone[i], p_alone[i] = o["embed"][0], o["probs"][0, :, 0]
    pl = np.where(lens <= 256, (lens + 63) // 64 * 64, (lens + 127) // 128 * 128)
    assert sorted(set(pl.tolist())) == [64, 128, 192, 256, 384, 512]
    for width in sorted(set(pl.tolist())):
        rows = np.flatnonzero(pl == width)
        W = int(lens[rows].max())
        o = eng.forward(np.ascontiguousarray(ids[rows[::-1], :W]), lens[rows[::-1]], want_embed=True)  # (reversed: another place in the batch, other batch mates)
        assert np.array_equal(o["embed"], alone[rows[::-1]]), width
        for streams in (1, 2):
            eng.set_streams(streams)
            _, _, ps = eng.bucketed_sweep(np.ascontiguousarray(ids[rows, :W]), lens[rows], 2, with_probs=True)  # three batches of two rows
            # (a batch of the sweep runs at ITS longest member's padded length: compare the rows whose batch runs at `width`)
            srt = np.argsort(lens[rows], kind="stable")
            at_width = np.zeros(len(rows), bool)
            for s0 in range(0, len(rows), 2):
                b = srt[s0:s0 + 2]
                L = int(lens[rows][b].max())
                at_width[b] = ((L + 63) // 64 * 64 if L <= 256 else (L + 127) // 128 * 128) == width
            assert at_width.any() and np.array_equal(ps[at_width], p_alone[rows][at_width]), (width, streams)
        eng.set_streams(2)
    whole = eng.forward_by_length(ids, lens, want_embed=True, min_tokens=1)
    assert np.array_equal(whole["embed"], alone)
    t1 = eng.forward_by_length_begin(ids, lens, want_embed=True, min_tokens=1)
    t2 = eng.forward_by_length_begin(ids[::-1].copy(), lens[::-1].copy(), want_embed=True, min_tokens=1)
    assert t1[0] == "pending" and t2[0] == "pending"
    r1, r2 = eng.forward_by_length_end(t1), eng.forward_by_length_end(t2)
    assert np.array_equal(r1["embed"], alone) and np.array_equal(r2["embed"], alone[::-1])
    eng.anchor_reset()
    # the switches of the default form's correction terms do not reach the safe form
    env = gu.engine_for(dk, wk, compute_dtype="safe", env={"MEMVUL_CLS_ASIDE": "0", "MEMVUL_QKV_ASIDE": "q"}, **kw)
    env.anchor_set(synth.make_anchor_bank(24))
    assert np.array_equal(env.forward_by_length(ids, lens, want_embed=True, min_tokens=1)["embed"], alone)
    env.anchor_reset()


# ---- 6. the default is untouched ---------------------------------------------------------------------------------------------------------------------------------

def test_the_default_form_is_untouched_by_a_visit_to_the_safe_form(gu):
    """6. The seeded inputs of test_gpu_parity.test_full_batch_properties: an engine whose form was never set, and a second one on which set_form("safe") then
    set_form("default") was called, give byte-equal outputs (and the safe form in between gives other bits: the switch does something)."""
    dk, wk = dict(layers=12), dict()
    dims, w = gu.weights_for(dk, wk)
    kw = dict(max_tokens=65536, max_batch=256, max_anchors=128)
    B, S, G = 256, 256, 124
    ids, lens = synth.make_ids(B, S, dims.vocab_size, ragged=False)
    aids, alens = synth.make_ids(G, 64, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=8)
    a = gu.engine_for(dk, wk, compute_dtype="precise", **kw)
    assert a.form == "default"
    a.anchor_reset(); a.anchor_append(aids, alens)
    oa = a.forward(ids, lens, want_embed=True)
    bank_a = a.anchor_get()
    a.anchor_reset()
    b = gu.engine_for(dk, wk, compute_dtype="precise", env={"MEMVUL_CLS_PRUNE": "1"}, **kw)  # (the default value: only a second engine)
    b.set_form("safe")
    assert b.form == "safe"
    b.anchor_reset(); b.anchor_append(aids, alens)
    os_ = b.forward(ids, lens, want_embed=True)
    b.set_form("default")
    assert b.form == "default"
    b.anchor_reset(); b.anchor_append(aids, alens)
    ob = b.forward(ids, lens, want_embed=True)
    assert np.array_equal(b.anchor_get(), bank_a)
    for k in ("logits", "probs", "best", "best_idx", "embed"):
        assert oa[k].tobytes() == ob[k].tobytes(), k
    assert not np.array_equal(os_["embed"], oa["embed"])
    gu.record("safe_vs_default_form_diffuse", max_logit_diff=float(np.abs(os_["logits"] - oa["logits"]).max()))
    b.anchor_reset()


# ---- 7. the fall-back --------------------------------------------------------------------------------------------------------------------------------------------

def _sink_warnings(rec, needle):
    return [str(r.message) for r in rec if needle in str(r.message)]


def test_on_sink_safe_switches_the_engine_and_redoes_the_call(gu, sink_refs, monkeypatch):
    """7. MEMVUL_ON_SINK=safe on mid_all_80_3001: the first call that meets the trip condition switches the form, warns once, leaves nothing of the default form
    behind — the bank, the call that tripped, the tickets in flight."""
    dims, w, ids, lens, aids, alens = _sink_case(sink_refs, "mid_all_80_3001")
    ref_lg = sink_refs["mid_all_80_3001_lg"]
    LA = int(alens.max())
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    safe = _sink_engine(dims, w, "safe")  # in the safe form from the start
    engines = [safe]
    try:
        safe.anchor_append(aids[:, :LA], alens)
        bank_safe = safe.anchor_get()
        out_safe = safe.forward(ids, lens)
        by_len_safe = safe.forward_by_length(ids, lens, min_tokens=256)
        rev_safe = safe.forward_by_length(ids[::-1].copy(), lens[::-1].copy(), min_tokens=256)
        monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
        # (a) six long anchors are 6 x 12 x 11 items: anchor_append is the call that trips, and the bank is encoded again
        e1 = _sink_engine(dims, w, "precise"); engines.append(e1)
        assert e1.form == "default"
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            e1.anchor_append(aids[:, :LA], alens)
            assert e1.form == "safe"
            out1 = e1.forward(ids, lens)
            e1.forward(ids, lens)
        told = _sink_warnings(rec, "SAFE form")
        assert len(told) == 1 and "encoded again" in told[0], [str(r.message) for r in rec]
        assert np.array_equal(e1.anchor_get(), bank_safe)
        assert np.array_equal(out1["logits"], out_safe["logits"])
        e = float(np.abs(out1["logits"] - ref_lg).max())
        gu.record("on_sink_fallback", case="mid_all_80_3001", logits_err=e)
        assert e <= LOGIT_TOL, e
        assert e1.attention_concentration()[2] > 0  # (the safe form keeps counting; it trips nothing: one warning above)
        # (b) a bank installed with anchor_set cannot be encoded again: kept, said so; forward is the call that trips and is redone
        e2 = _sink_engine(dims, w, "precise"); engines.append(e2)
        e2.anchor_set(bank_safe)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out2 = e2.forward(ids, lens)
        told = _sink_warnings(rec, "SAFE form")
        assert len(told) == 1 and "KEPT" in told[0], [str(r.message) for r in rec]
        assert e2.form == "safe" and np.array_equal(e2.anchor_get(), bank_safe)
        assert np.array_equal(out2["logits"], out_safe["logits"])
        # (c) begin, begin, end, end across the trip: both tickets come back with the bits of the safe form
        e3 = _sink_engine(dims, w, "precise"); engines.append(e3)
        e3.anchor_set(bank_safe)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            t1 = e3.forward_by_length_begin(ids, lens, min_tokens=256)
            t2 = e3.forward_by_length_begin(ids[::-1].copy(), lens[::-1].copy(), min_tokens=256)
            assert t1[0] == "pending" and t2[0] == "pending" and e3.form == "default"
            r1 = e3.forward_by_length_end(t1)
            assert e3.form == "safe"
            r2 = e3.forward_by_length_end(t2)
        assert len(_sink_warnings(rec, "SAFE form")) == 1
        for k in ("logits", "probs", "best", "best_idx"):
            assert np.array_equal(r1[k], by_len_safe[k]) and np.array_equal(r2[k], rev_safe[k]), k
    finally:
        for e_ in engines:
            e_.close()


def test_on_sink_safe_leaves_a_delimiter_sink_alone_and_warn_is_the_parents_behaviour(gu, sink_refs, monkeypatch):
    """7. sep_all_80_3001 under MEMVUL_ON_SINK=safe never switches (the special rows cover it); under MEMVUL_ON_SINK=warn (and unset) mid_all_80_3001 gets the one
    warning it always got, and stays in the default form."""
    monkeypatch.setenv("MEMVUL_ON_SINK", "safe")
    dims, w, ids, lens, aids, alens = _sink_case(sink_refs, "sep_all_80_3001")
    eng = _sink_engine(dims, w, "precise")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            eng.anchor_append(aids[:, :int(alens.max())], alens)
            eng.forward(ids, lens)
            eng.encode(ids, lens)
        assert eng.form == "default" and not _sink_warnings(rec, "ordinary token")
    finally:
        eng.close()
    dims, w, ids, lens, aids, alens = _sink_case(sink_refs, "mid_all_80_3001")
    for setting in ("warn", None):
        if setting is None:
            monkeypatch.delenv("MEMVUL_ON_SINK")
        else:
            monkeypatch.setenv("MEMVUL_ON_SINK", setting)
        eng = _sink_engine(dims, w, "precise")
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                eng.encode(ids, lens)
                eng.encode(ids, lens)
            told = _sink_warnings(rec, "ONE ordinary token")
            assert len(told) == 1 and "MEMVUL_CLS_ASIDE=0 MEMVUL_QKV_ASIDE=qkv is the most conservative form" in told[0] and "SAFE form" not in told[0], told
            assert eng.form == "default"
        finally:
            eng.close()


# ---- 8. strict parsing -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_new_switches_are_parsed_strictly(gu, monkeypatch):
    from memvul_amd.binding import Engine

    dims, w = gu.weights_for(L2, WK)
    kw = dict(vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=4096, max_batch=16, max_anchors=16)
    monkeypatch.delenv("MEMVUL_ON_SINK", raising=False)
    monkeypatch.setenv("MEMVUL_FORM", "sfae")
    with pytest.raises(RuntimeError, match="MEMVUL_FORM"):
        Engine(0, **kw)
    monkeypatch.setenv("MEMVUL_FORM", "safe")
    eng = Engine(0, **kw)
    try:
        with pytest.raises(RuntimeError, match="MEMVUL_FORM"):
            eng.load_state_dict(w, "f16")
    finally:
        eng.close()
    eng = Engine(0, **kw)
    try:
        eng.load_state_dict(w, "precise")
        assert eng.form == "safe"  # the switch alone selects the form: how bench.py measures it
    finally:
        eng.close()
    monkeypatch.delenv("MEMVUL_FORM")
    eng = Engine(0, **kw)
    try:
        eng.load_state_dict(w, "f16")
        with pytest.raises(RuntimeError, match="MV_F16"):
            eng.set_form("safe")
        assert eng.form == "default"
        with pytest.raises(ValueError):
            eng.set_form("safest")
    finally:
        eng.close()
    monkeypatch.setenv("MEMVUL_ON_SINK", "maybe")
    with pytest.raises(ValueError, match="MEMVUL_ON_SINK"):
        Engine(0, **kw)
