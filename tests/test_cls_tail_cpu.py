"""The bounds of tests/cls_tail_kit.py, fixed on the CPU: a numpy emulation of attention_cls_kernel, dense768_kernel, cls_gather_kernel and ln_kernel<true> in the
kernels' own order and precision (fp32 fma chains per lane group and the three xor-shuffle adds; 8 waves x ascending k summed in wave order; P rounded to fp16 or
not) has to stay inside every bound on every element — the condition that keeps the bounds honest — and each fault of kit.MUTATIONS has to exceed its bound on at
least one element wherever it is active.  Where a form's bound cannot see a fault, UNSEEN names it with the reason and the test asserts that too (a bound that
starts to see it has to take the entry out).

Operands: random, at the shapes of tests/test_cls_tail_gpu.py — a sink on key 1 (80 % of the row's mass), |v| outliers on the sink key, LayerNorm outlier
dimensions (27 x the bulk) in the stream rows."""
import numpy as np
import pytest

import cls_tail_kit as kit

_f32, _f16, _f64 = np.float32, np.float16, np.float64

# (padded length, lengths): one to eight 64-key PV blocks, lengths on the mask's edges and below 16
ATTN_CASES = {
    "s64": (64, (2, 3, 7, 9, 63, 64)),
    "s128": (128, (65, 127, 128, 9)),
    "s192": (192, (191, 192, 64, 3)),
    "s512": (512, (511, 512, 65, 7)),
}
FORMS = ("precise", "precise_vlo", "f16", "safe")  # precise_vlo: with the vlo_sp term (padded length > 128 in the engine)

# (form, mutation) -> why this form's bound cannot see the fault
UNSEEN = {
    ("f16", "rounded_sum"): "bound_one_plane allows every p_k half an fp16 ulp, in any direction: a sum of the rounded p differs by less",
    ("safe", "rounded_sum"): "the safe form rounds no p: the rounded and the unrounded sum are the same numbers",
}
NO_VLO = "this form passes no vlo_sp"


def attn_operands(Sp, lens, seed, sink=True):
    """q [B, 12, 64] fp32, k, v hi and lo planes [B, 12, Sp, 64] fp16, vlo_sp [B, 12, 64, 2] fp16.  Key 1 (the engine's [SEP] row) takes ~80 % of the mass where
    the sequence is long enough to matter, and its V is an outlier (8 x the bulk); padded keys hold finite values like any other."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    q = rng.standard_normal((B, 12, 64)) * 0.6
    k = rng.standard_normal((B, 12, Sp, 64)) * 0.6
    v = rng.standard_normal((B, 12, Sp, 64))
    if sink:
        for b, n in enumerate(lens):
            # raise the score of key 1 to log(4 (n - 1)) above the bulk: p_1 ~ 0.8
            qq = q[b] / (q[b] ** 2).sum(-1, keepdims=True)
            k[b, :, 1] = qq * (np.log(4.0 * max(n - 1, 1)) + 1.0)
        v[:, :, 1] *= 8.0
    k_hi, v_hi = k.astype(_f16), v.astype(_f16)
    k_lo, v_lo = (k - k_hi.astype(_f64)).astype(_f16), (v - v_hi.astype(_f64)).astype(_f16)
    vlo_sp = ((v[:, :, :2] - v_hi[:, :, :2].astype(_f64)) * 2048.0).astype(_f16).transpose(0, 1, 3, 2)
    return q.astype(_f32), k_hi, k_lo, v_hi, v_lo, np.ascontiguousarray(vlo_sp)


def attn_share(form, Sp, lens, seed, mutation=None):
    """|emulation - model| / bound [B, 12, 64] of one form, the reference and the bound exactly as kit.check_tail forms them from an engine's taps."""
    q, k_hi, k_lo, v_hi, v_lo, vlo_sp = attn_operands(Sp, lens, seed)
    lens = np.asarray(lens)
    q64, k64, v64 = q.astype(_f64), k_hi.astype(_f64), v_hi.astype(_f64)
    sp_keys = np.tile(np.array([0, 1]), (len(lens), 1))
    if form == "safe":
        got = kit.emulate_attention_cls(q, k_hi, v_hi, lens, lo=True, k_lo=k_lo, v_lo=v_lo, mutation=mutation)
        ref, bnd = kit.attn_safe_model(q64, k64 + k_lo.astype(_f64), v64 + v_lo.astype(_f64), lens)
    elif form == "f16":
        got = kit.emulate_attention_cls(q, k_hi, v_hi, lens, ctx16=True, mutation=mutation)
        ref, bnd = kit.attn_f16_model(q64, k64, v64, lens)
    else:
        vl = vlo_sp if form == "precise_vlo" else None
        got = kit.emulate_attention_cls(q, k_hi, v_hi, lens, vlo_sp=vl, mutation=mutation)
        ref, bnd = kit.attn_exact_model(q64, k64, v64, lens, None if vl is None else vl.astype(_f64), sp_keys)
    assert np.isfinite(got).all()
    return kit.share(got, ref, bnd)


def attn_active(mutation, lens, Sp):
    """bool [B]: the sequences in which the fault changes anything."""
    lens = np.asarray(lens)
    return {"mask_len_plus_1": lens < Sp, "group_neighbour_head": lens > 8}.get(mutation, np.ones(len(lens), bool))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_emulation_stays_inside_the_bound(case, form):
    Sp, lens = ATTN_CASES[case]
    r = attn_share(form, Sp, lens, seed=11)
    print(f"attention_cls {form} {case}: worst {r.max():.3f} rms {np.sqrt((r ** 2).mean()):.3f}")
    assert r.max() <= 1.0, (r.max(), np.unravel_index(r.argmax(), r.shape))


@pytest.mark.parametrize("mutation", kit.ATTN_MUTATIONS)
@pytest.mark.parametrize("form", FORMS)
def test_attention_bounds_catch_the_faults(form, mutation):
    for case, (Sp, lens) in ATTN_CASES.items():
        if mutation.startswith("vlo_sp") and form != "precise_vlo":
            continue  # NO_VLO: the term does not exist in this form (encoder_pass.h special_v_lo), so the fault has nothing to act on
        r = attn_share(form, Sp, lens, seed=11, mutation=mutation)
        per_seq = r.reshape(len(lens), -1).max(-1)
        act = attn_active(mutation, lens, Sp)
        if (form, mutation) in UNSEEN:
            assert per_seq.max() <= 1.0, (UNSEEN[(form, mutation)], case, per_seq)
            continue
        assert (per_seq[act] > 1.0).all(), (form, mutation, case, per_seq, act)
        assert (per_seq[~act] <= 1.0).all(), (form, mutation, case, per_seq, act)


# ---- dense768 ------------------------------------------------------------------------------------------------------------------------------------------------------------

def stream_rows(B, K, seed, outliers=True):
    """Rows like the tail's: unit bulk, LayerNorm outlier dimensions of 27 x (two per row of 768)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, K))
    if outliers:
        x[:, 5::384] *= 27.0
    return x.astype(_f32)


DENSE_CASES = [(act, KT, N, B) for B in (1, 5, 33) for act, KT, N in
               ((kit.ACT_ID, 768, 768), (kit.ACT_RES, 768, 768), (kit.ACT_GELU, 768, 3072), (kit.ACT_RES, 3072, 768), (kit.ACT_TANH, 768, 768), (kit.ACT_RELU, 768, 512))]


def dense_operands(act, KT, N, B, seed=3):
    rng = np.random.default_rng(seed)
    x = stream_rows(B, KT, seed)
    W = (rng.standard_normal((N, KT)) * 0.03).astype(_f32)
    bias = (rng.standard_normal(N) * 0.5).astype(_f32)   # (distinct per column: a bias of the wrong column shows)
    res = stream_rows(B, N, seed + 1) if act == kit.ACT_RES else None
    return x, W, bias, res


def dense_share(act, KT, N, B, mutation=None):
    x, W, bias, res = dense_operands(act, KT, N, B)
    got = kit.emulate_dense768(x, W, bias, act, res, mutation)
    m, bnd, _ = kit.dense_model(x.astype(_f64), W.astype(_f64), bias.astype(_f64), act, None if res is None else res.astype(_f64))
    return kit.share(got, m, bnd)


@pytest.mark.parametrize("act,KT,N,B", DENSE_CASES)
def test_dense768_emulation_stays_inside_the_bound(act, KT, N, B):
    assert kit.dense_roundings(768, kit.ACT_ID) == 96 + 7 + 1 and kit.dense_roundings(3072, kit.ACT_RES) == 384 + 7 + 2
    r = dense_share(act, KT, N, B)
    print(f"dense768 act {act} K {KT} N {N} B {B}: worst {r.max():.3f} rms {np.sqrt((r ** 2).mean()):.3f}")
    assert r.max() <= 1.0


@pytest.mark.parametrize("mutation", kit.DENSE_MUTATIONS)
def test_dense768_bounds_catch_the_faults(mutation):
    for act, KT, N, B in DENSE_CASES:
        active = {"chunk_dropped": KT == 3072, "clamped_row_stored": B >= 2, "residual_omitted": act == kit.ACT_RES}.get(mutation, True)
        r = dense_share(act, KT, N, B, mutation)
        if not active:  # (a 96-chunk is the whole share of a wave at K = 768; one row has no other row to take; no residual to omit: the emulation is the unmutated one)
            assert r.max() <= 1.0
            continue
        rows = r.max(-1)
        if mutation == "clamped_row_stored":
            assert rows[-1] > 1.0 and (rows[:-1] <= 1.0).all(), (act, KT, B, rows)
        else:
            assert (rows > 1.0).all(), (mutation, act, KT, N, B, rows)  # every row: a defect in one sequence cannot hide behind the others


# ---- gather and LayerNorm ------------------------------------------------------------------------------------------------------------------------------------------------

def gather_operands(B, Sp, x8, seed=5):
    """The raw stream of a pass as hi + low parts with its vstats: per token for MV_F16 (xlo), compact 2^11 x for MV_F16X8 (sp_lo [2 B])."""
    rng = np.random.default_rng(seed)
    x = stream_rows(B * Sp, 768, seed).astype(_f64) * (1.0 + rng.random((B * Sp, 1))) + rng.standard_normal((B * Sp, 1)) * 0.3
    hi = x.astype(_f16)
    rest = x - hi.astype(_f64)
    if x8:
        lo = np.stack([rest[np.arange(B) * Sp], rest[np.arange(B) * Sp + 1]], 1).reshape(2 * B, 768)
        lo = (lo * 2048.0).astype(_f16)
        stored = hi.astype(_f64)
        stored[np.arange(B) * Sp] += lo[0::2].astype(_f64) / 2048.0
        stored[np.arange(B) * Sp + 1] += lo[1::2].astype(_f64) / 2048.0
    else:
        lo = rest.astype(_f16)
        stored = hi.astype(_f64) + lo.astype(_f64)
    t = stored.reshape(B * Sp, 3, 256)
    vst = np.stack([t.sum(-1), (t ** 2).sum(-1)], -1).astype(_f32)
    g = (1.0 + 0.1 * rng.standard_normal(768)).astype(_f32)
    b = (0.1 * rng.standard_normal(768)).astype(_f32)
    return hi, lo, vst, g, b


def gather_share(B, Sp, x8, mutation=None):
    hi, lo, vst, g, b = gather_operands(B, Sp, x8)
    scale = 2.0 ** -11 if x8 else 1.0
    c32, c16 = kit.emulate_gather(hi, lo, scale, vst, g, b, Sp, mutation)
    rows = np.arange(B) * Sp
    lo_cls = lo[0::2] if x8 else lo[rows]
    m, bnd = kit.gather_model(hi[rows].astype(_f64), lo_cls.astype(_f64), scale, vst[rows].astype(_f64), g.astype(_f64), b.astype(_f64))
    assert np.array_equal(c16, c32.astype(_f16))
    return kit.share(c32, m, bnd)


@pytest.mark.parametrize("x8", [True, False], ids=["sp_lo", "xlo"])
@pytest.mark.parametrize("B,Sp", [(1, 64), (5, 128), (33, 64)])
def test_gather_emulation_stays_inside_the_bound_and_the_faults_do_not(B, Sp, x8):
    r = gather_share(B, Sp, x8)
    print(f"gather {'sp_lo' if x8 else 'xlo'} B {B}: worst {r.max():.3f} rms {np.sqrt((r ** 2).mean()):.3f}")
    assert r.max() <= 1.0
    for mutation in kit.GATHER_MUTATIONS:
        if mutation == "sp_lo_unscaled" and not x8:
            continue  # MV_F16's low part is the lo plane itself: there is no scale to forget
        rows = gather_share(B, Sp, x8, mutation).max(-1)
        assert (rows > 1.0).all(), (mutation, rows)


@pytest.mark.parametrize("B", [1, 5, 33])
def test_layernorm_emulation_stays_inside_the_bound(B):
    rng = np.random.default_rng(9)
    x = stream_rows(B, 768, 21) * _f32(1.7) + _f32(0.4)
    g = (1.0 + 0.1 * rng.standard_normal(768)).astype(_f32)
    b = (0.1 * rng.standard_normal(768)).astype(_f32)
    o32, o16 = kit.emulate_ln(x, g, b)
    m, bnd = kit.ln_model(x.astype(_f64), g.astype(_f64), b.astype(_f64))
    r = kit.share(o32, m, bnd)
    print(f"layernorm B {B}: worst {r.max():.3f}")
    assert r.max() <= 1.0
    # the faults a LayerNorm on B rows can have: the statistics of the neighbouring row, gamma / beta of the neighbouring column
    if B >= 2:
        assert (kit.share(np.roll(o32, 1, axis=0), m, bnd).max(-1) > 1.0).all()
    assert (kit.share(kit.emulate_ln(x, np.roll(g, 1), b)[0], m, bnd).max(-1) > 1.0).all()


def test_every_listed_fault_is_covered():
    """The list of the kit against the tests above: each mutation is detected, or named in UNSEEN / as absent from a form with the reason."""
    assert set(kit.MUTATIONS) == set(kit.ATTN_MUTATIONS) | set(kit.DENSE_MUTATIONS) | set(kit.GATHER_MUTATIONS) and len(kit.MUTATIONS) == 15
    assert all(m in kit.ATTN_MUTATIONS and f in FORMS and why for (f, m), why in UNSEEN.items()) and NO_VLO
