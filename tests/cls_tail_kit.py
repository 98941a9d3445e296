"""Shared pieces of the [CLS]-tail tests (tests/test_cls_tail_cpu.py, tests/test_cls_tail_gpu.py): every launch of the pruned last layer's tail
(encoder_pass.h pruned_last_layer / cls_tail_f32 / cls_tail_f16 / pool_head) against a float64 model formed from THAT LAUNCH'S OWN operands — the tail taps of the
development build (MEMVUL_DEBUG_TAIL=1, include/memvul_hip.h buffers 22 - 34) and the taps of the tail's inputs — never from the previous model's output.  Plain
module: no fixtures, no GPU.

The bounds are derived from the roundings the kernels perform, not measured (u = 2^-24, half an fp32 ulp relative):

  gather      big path: y = fma(lo, scale, hi) (u |y|), d = y - mean, t = d rstd, out = fma(t, g, b): one rounding each, with mean and rstd from
              common.h ln_from_partials in fp32 (gather_bound).  Small path: a copy, exact.  c16 = fp16(c32) exactly (big) or the copied x16.
  dense768    pre-activation: R x u x sum_k |x_k w_k| with R = KT / 8 (a wave's sequential accumulations, ascending k) + 7 (the cross-wave adds, in wave order)
              + 1 (bias) [+ 1: the residual of ACT 4] (dense_roundings).  GELU: 1e-6 max(1, |ref|) (tests/test_gelu_arithmetic.py) + 1.13 x that; tanh: that
              + 2^-20 |out| (a cap above any libm's few ulp); ReLU, identity, residual: that.
  fp16 GEMMs  of cls_tail_f16: gemm_stage_kit's storage rounding + ACC x rms(pre-activation) (fp16 operands, fp32 accumulation); the two residual launches park
              bias + residual in the accumulator and get gemm_stage_kit.allowance's residual term for it (skinny_model).
  LayerNorm   ln_kernel<true> on B rows: mean over 768 (<= 12 roundings of a partial sum), the centred variance by fma, 1 / sqrtf, then the expression of the
              gather (ln_bound).  c16 = fp16(c32) exactly.
  attention   attention_cls_kernel, one query row:
              <false>, fp32 context (MV_F16X8 default form): the model rounds the query and exp(s - max) to fp16 as the kernel does; an element of P gets a
                one-ulp allowance only where its fp32 error (score accumulation, the common maximum, __expf) reaches a rounding tie; + the fp32 accumulation of
                P V and of the row sum; + the vlo_sp term wherever the engine passes it.  No 2^-11 |ref| store term (attn_bound_exact).
              <false>, fp16 context (MV_F16): stage_kit.bound_one_plane.
              <true> (safe form): nothing of the row is rounded: stage_kit.bound_two_plane without the store term, 2^-14 max |V|.
tests/test_cls_tail_cpu.py holds a numpy emulation of each kernel (its own order and precision) inside every bound on every element, and shows the faults the
bounds catch (MUTATIONS)."""
import numpy as np
from scipy.special import erfc

import gemm_stage_kit as gsk
import stage_kit as sk

H, INTER, HEADS, HD, PROJ = 768, 3072, 12, 64, 512
U = 2.0 ** -24
LN_EPS = 1e-12
_f32, _f16, _f64 = np.float32, np.float16, np.float64

# the delimiter-sink model of the monitor-parity tests (scripts/make_monitor_refs.py sep_cls_80: seed 5005, 80 % of the [CLS] row's mass on [SEP]) at 2 and 4 layers:
# the gains are synth.calibrate_sink(BertDims(layers=4, vocab_size=2048), 5005, 0.8, token="sep", rows="cls", n=2, seq_len=128, **SINK_KW) — calibrated layer
# by layer, so the 2-layer model's are the first two
SINK_KW = dict(qk_scale=2.0, match_scale=29.0, trained_like=True)
SINK_SEED = 5005
SINK_GAINS = (0.7030029296875, 0.6829833984375, 0.5572509765625, 0.5023193359375)


def f32(x):
    return np.asarray(x, _f64).astype(_f32).astype(_f64)


def f16(x):
    return np.asarray(x, _f64).astype(_f16).astype(_f64)


def gelu64(x):
    return x * 0.5 * erfc(-x / np.sqrt(2.0))


# ---- the weights of the tail, as weights.h stores them ----------------------------------------------------------------------------------------------------------

def tail_weights(w, layers, fp16_ops):
    """float64 matrices [N, K] of the last layer's tail: W_q / b_q with the folded 1 / 8, W_o, W_1, W_2 (fp32 as wqT32 ... hold them; fp16_ops: rounded to
    fp16 as MV_F16's wqkv, wo, w1, w2 are), the LayerNorms, the pooler W_p / b_p and the header W_h / b_h (None without one)."""
    from oracle import memvul_oracle as orc

    p = orc.PFX + f"encoder.layer.{layers - 1}."
    g = lambda k: np.asarray(w[k], _f32).astype(_f64)  # noqa: E731
    rw = f16 if fp16_ops else (lambda x: x)
    out = dict(wq=rw(f32(g(p + "attention.self.query.weight") * 0.125)), bq=f32(g(p + "attention.self.query.bias") * 0.125),
               wo=rw(g(p + "attention.output.dense.weight")), bo=g(p + "attention.output.dense.bias"),
               w1=rw(g(p + "intermediate.dense.weight")), b1=g(p + "intermediate.dense.bias"),
               w2=rw(g(p + "output.dense.weight")), b2=g(p + "output.dense.bias"),
               ln1g=g(p + "attention.output.LayerNorm.weight"), ln1b=g(p + "attention.output.LayerNorm.bias"),
               ln2g=g(p + "output.LayerNorm.weight"), ln2b=g(p + "output.LayerNorm.bias"),
               wp=g("_bert_pooler.pooler.dense.weight"), bp=g("_bert_pooler.pooler.dense.bias"), wh=None, bh=None)
    if layers >= 2:
        q = orc.PFX + f"encoder.layer.{layers - 2}.output.LayerNorm."
    else:
        q = orc.PFX + "embeddings.LayerNorm."
    out["pend_g"], out["pend_b"] = g(q + "weight"), g(q + "bias")
    if "_projector_single._linear_layers.0.weight" in w:
        out["wh"], out["bh"] = g("_projector_single._linear_layers.0.weight"), g("_projector_single._linear_layers.0.bias")
    return out


# ---- gather --------------------------------------------------------------------------------------------------------------------------------------------------------

def partial_stats64(vst):
    """vstats [B, 3, 2] -> mean, var, e2 = E[x^2] in float64 by the rule of common.h ln_from_partials."""
    s = np.asarray(vst, _f64)
    s1, s2 = s[:, :, 0].sum(-1), s[:, :, 1].sum(-1)
    mean, e2 = s1 / H, s2 / H
    return mean[:, None], np.maximum(e2 - mean * mean, 0.0)[:, None], e2[:, None], (np.abs(s[:, :, 0]).sum(-1) / H)[:, None]


def _ln_expr_bound(y, dy, mean, dmean, rstd, rel_rstd, g, out):
    """The roundings of out = fma((y - mean) rstd, g, b) in fp32, given |error| of y and mean and the relative error of rstd."""
    d = y - mean
    dd = U * np.abs(d) + dy + dmean
    t = d * rstd
    dt = U * np.abs(t) + rstd * dd + np.abs(t) * rel_rstd
    return U * np.abs(out) + np.abs(g) * dt


def gather_model(hi, lo, lo_scale, vst, g, b):
    """Big path: (c32 model, bound).  hi, lo [B, 768] float64 (the [CLS] row's fp16 hi plane and its low part: sp_lo = 2^11 x, scale 2^-11, in MV_F16X8; xlo,
    scale 1, in MV_F16), vst [B, 3, 2] that row's vstats."""
    y = hi + lo * lo_scale
    mean, var, e2, a1 = partial_stats64(vst)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    out = (y - mean) * rstd * g + b
    dmean = 4.0 * U * a1                                     # two adds of the partial sums, the product with the rounded 1 / 768
    dvar = 12.0 * U * (e2 + mean * mean)                     # s2 (2), x 1 / 768 (2), mean^2 (1 + 2 x 4 from mean), the difference (1): 12 u (E[x^2] + mean^2) covers them
    rel_rstd = 0.5 * dvar / (var + LN_EPS) + 3.0 * U         # + the rounding of var + eps and v_rsq_f32's 1 ulp
    return out, _ln_expr_bound(y, U * np.abs(y), mean, dmean, rstd, rel_rstd, g, out)


def ln_model(x, g, b):
    """ln_kernel<true> of the rows x [B, 768] (exact fp32 inputs): (model, bound)."""
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    out = d * rstd * g + b
    ma = np.abs(x).mean(-1, keepdims=True)
    dmean = 12.0 * U * ma + U * np.abs(mean)                 # 5 adds in the lane, 6 butterfly levels, x 1 / 768
    md = np.abs(d).mean(-1, keepdims=True)
    dvar = 20.0 * U * var + 2.0 * dmean * md + dmean ** 2    # a = x - mean (u |a| each, twice in a^2), the fma chain and the butterfly (<= 18 u), the shifted mean
    rel_rstd = 0.5 * dvar / (var + LN_EPS) + 6.0 * U         # x 1 / 768, + eps, sqrtf, the division
    return out, _ln_expr_bound(x, 0.0, mean, dmean, rstd, rel_rstd, g, out)


# ---- dense768_kernel -------------------------------------------------------------------------------------------------------------------------------------------------

ACT_TANH, ACT_RELU, ACT_ID, ACT_GELU, ACT_RES = 0, 1, 2, 3, 4
TANH_CAP = 2.0 ** -20
GELU_ABS = 1e-6
GELU_SLOPE = 1.13


def dense_roundings(KT, act):
    """Sequential fp32 roundings an output element passes: a wave's KT / 8 accumulations (one per k: v_mfma_f32_32x32x2_f32 adds its two k one after the
    other, lanes 0 - 31 carry the even k), the 7 cross-wave adds, the bias, the residual of ACT 4."""
    return KT // 8 + 7 + 1 + (1 if act == ACT_RES else 0)


def dense_model(x, W, bias, act, res=None):
    """(model, bound, pre-activation bound) of dense768_kernel<act, KT = x.shape[1]>: x [B, K], W [N, K], all float64 holding fp32 values."""
    pre = x @ W.T + bias
    mag = np.abs(x) @ np.abs(W).T
    bp = dense_roundings(x.shape[1], act) * U * mag
    if act == ACT_TANH:
        out = np.tanh(pre)
        return out, bp + TANH_CAP * np.abs(out), bp
    if act == ACT_RELU:
        return np.maximum(pre, 0.0), bp, bp
    if act == ACT_GELU:
        out = gelu64(pre)
        return out, GELU_ABS * np.maximum(1.0, np.abs(out)) + GELU_SLOPE * bp, bp
    if act == ACT_RES:
        return pre + res, bp, bp
    return pre, bp, bp


# ---- the fp16 skinny GEMMs of cls_tail_f16 -----------------------------------------------------------------------------------------------------------------------------

def skinny_model(a16, W16, bias, kind, res=None):
    """(model, bound) of a launch_small GEMM on B rows: a16 [B, K] and W16 [N, K] fp16 values, fp32 accumulation.  kind "f32" (Q projection: fp32 out), "res"
    (+ bias + the fp32 residual, fp32 out), "gelu" (fp16 out).  gemm_stage_kit's form: storage rounding + ACC x rms(pre-activation)."""
    pre = a16 @ W16.T + bias
    acc = gsk.ACC * float(np.sqrt((pre ** 2).mean()))
    if kind == "gelu":
        out = gelu64(pre)
        return out, GELU_ABS * np.maximum(1.0, np.abs(out)) + GELU_SLOPE * acc + gsk.half_ulp16(f16(out)) * (1.0 + 2.0 ** -10)
    if kind == "f32":
        return pre, acc + 2.0 * U * np.abs(pre)               # the epilogue's bias add, the fp32 store
    # EPI_RES parks bias + residual — the element's full magnitude — in the accumulator BEFORE the K loop (gemm.h), so every later rounding of the accumulator
    # is a rounding of that magnitude whatever the products add: gemm_stage_kit.allowance's residual term, 3 sigma of a random walk of R roundings of half an
    # fp32 ulp, R = ROUNDINGS_PER_MFMA x K / 32 (one per 4 K-elements; this launch has the fp16 sweep alone).  The rms cannot stand for an element of 27 rms
    # (LayerNorm outlier dimensions).
    out = pre + res
    R = gsk.ROUNDINGS_PER_MFMA * (a16.shape[1] // 32)
    return out, acc + 3.0 * np.sqrt(R / 12.0) * 2.0 ** -23 * np.maximum(np.abs(out), np.abs(res + bias)) + U * np.abs(out)


# ---- attention_cls_kernel --------------------------------------------------------------------------------------------------------------------------------------------

def _scores64(q, k, lens):
    """q [B, H, D], k [B, H, S, D] -> scores [B, H, S] with the additive mask, and sum_d |q_d k_d|."""
    s = np.einsum("bhd,bhkd->bhk", q, k)
    mag = np.einsum("bhd,bhkd->bhk", np.abs(q), np.abs(k))
    S = k.shape[2]
    masked = np.arange(S)[None, :] >= np.asarray(lens)[:, None]
    return s + np.where(masked, -10000.0, 0.0)[:, None, :], mag, masked


def _attention_terms_one_row(q, k, v, lens):
    """stage_kit.attention_terms64 for the one query row (token 0) of every (sequence, head): q [B, 12, 64] placed in row 0 of a zero Q (the function reads
    the padded length off Q); of the terms [B, 12, S, 64] row 0 is the tail's."""
    qq = np.zeros(k.shape)
    qq[:, :, 0] = q
    return sk.attention_terms64(qq, k, v, lens)


def attn_safe_model(q, k, v, lens):
    """<true>: fp32 query, K and V as hi + lo (already summed), P unrounded: (ref [B, 12, 64], bound = 2^-14 max |V| per (sequence, head))."""
    t = _attention_terms_one_row(q, k, v, lens)
    return t["ref"][:, :, 0], np.broadcast_to(2.0 ** -14 * t["vmax"][:, :, 0], t["ref"][:, :, 0].shape)


def attn_f16_model(q, k, v, lens):
    """<false> with the fp16 context (MV_F16): the query rounded to fp16 as the kernel rounds it; stage_kit.bound_one_plane."""
    t = _attention_terms_one_row(f16(q), k, v, lens)
    return t["ref"][:, :, 0], sk.bound_one_plane(t)[:, :, 0]


def attn_exact_model(q, k, v, lens, vlo_sp=None, sp_keys=None):
    """<false> with the fp32 context (MV_F16X8, default form).  q [B, 12, 64] fp32 values, k, v [B, 12, S, 64] fp16 values; vlo_sp [B, 12, 64, 2] (2^11 x the
    low parts of V of the keys sp_keys [B, 2]) or None.  The model rounds q and exp(s - max) to fp16; returns (ref, bound) [B, 12, 64]."""
    B, Hh, S, D = k.shape
    q16 = f16(q)
    s, mag, masked = _scores64(q16, k, lens)
    mx = s.max(-1, keepdims=True)
    p = np.exp(s - mx)
    p16 = f16(p)
    psum = p.sum(-1, keepdims=True)
    num = np.einsum("bhk,bhkd->bhd", p16, v)
    av = np.abs(v)
    mag_pv = np.einsum("bhk,bhkd->bhd", p16, av)
    if vlo_sp is not None:
        bi = np.arange(B)
        for j in (0, 1):
            pj = p16[bi, :, np.asarray(sp_keys)[:, j]]                      # [B, H]
            num = num + pj[:, :, None] * vlo_sp[..., j] / 2048.0
            mag_pv = mag_pv + pj[:, :, None] * np.abs(vlo_sp[..., j]) / 2048.0
    ref = num / psum
    # the fp32 error of an element of P before its fp16 rounding: the score (8 fma, 3 shuffle adds, the mask add: 12 u sum |q k|), the common maximum (the
    # largest such error of the row), __expf = exp2(x log2 e): the rounded product moves the exponent by |x| 2^-24 log2 e, v_exp_f32 by 1 ulp
    ds = 12.0 * U * mag
    eps = ds + ds.max(-1, keepdims=True) + np.abs(s - mx) * 2.0 ** -23 + 2.0 ** -22
    eps = np.where(masked[:, None, :], 0.0, eps)                                        # (exp(-10000 + ...) = 0 exactly, both sides)
    tie = (p * (1.0 - eps)).astype(_f16) != (p * (1.0 + eps)).astype(_f16)
    ulp = np.spacing(np.maximum(p16, 2.0 ** -24).astype(_f16)).astype(_f64)
    b_tie = np.einsum("bhk,bhkd->bhd", np.where(tie, ulp, 0.0), av)
    rn = S // 8 + 3 + 2 + 1                                                 # S / 8 fma per lane, 3 shuffle adds, the vlo_sp fma pair, x inv
    rd = S // 64 + 6 + 2                                                    # the row sum: per lane, the wave reduction, 1 / x
    rel_sum = (p * eps).sum(-1, keepdims=True) / psum                       # the row sum takes the UNROUNDED p with their fp32 errors
    return ref, (b_tie + rn * U * mag_pv) / psum + np.abs(ref) * (rd * U + rel_sum)


# ---- numpy emulations of the kernels: their own order and precision ----------------------------------------------------------------------------------------------------

ATTN_MUTATIONS = ("mask_len_plus_1", "mask_len_minus_1", "group_neighbour_head", "pv_block_dropped", "rounded_sum", "vlo_sp_omitted", "vlo_sp_2_10")
DENSE_MUTATIONS = ("wave_dropped", "chunk_dropped", "clamped_row_stored", "bias_n_plus_32", "residual_omitted")
GATHER_MUTATIONS = ("row_plus_1", "sp_lo_unscaled", "neighbour_stats")
MUTATIONS = ATTN_MUTATIONS + DENSE_MUTATIONS + GATHER_MUTATIONS


def _fma(a, b, c):
    return (a.astype(_f64) * b.astype(_f64) + c.astype(_f64)).astype(_f32)


def _xor_sum(x):
    """x [..., n] fp32 -> the butterfly sum over the last axis (xor-shuffle adds 1, 2, 4, ...), every lane's value [..., n]."""
    n = x.shape[-1]
    idx = np.arange(n)
    off = 1
    while off < n:
        x = (x + x[..., idx ^ off]).astype(_f32)
        off *= 2
    return x


def emulate_attention_cls(q, k, v, lens, lo=False, k_lo=None, v_lo=None, vlo_sp=None, ctx16=False, mutation=None):
    """attention_cls_kernel<lo> in its own order: q [B, 12, 64] fp32, k, v [B, 12, S, 64] fp16 (engine row order: keys 0 and 1 are the special rows), lens [B].
    Scores: per lane (key, 8-dim chunk c) an fp32 fma chain over its 8 dims, the three xor-shuffle adds over c, the -10000 mask; one maximum; p = exp(s - max)
    in fp32, the row sum from the fp32 p, P rounded to fp16 (not in the safe form); PV: per lane (dim, 8-key chunk c) an fma chain over the 64-key blocks in
    ascending order, the three xor-shuffle adds; + the vlo_sp pair; x 1 / sum.  Returns [B, 12, 64] fp32 (ctx16: rounded to fp16)."""
    assert mutation is None or mutation in ATTN_MUTATIONS
    B, Hh, S, D = k.shape
    lens = np.asarray(lens)
    qv = q.astype(_f32) if lo else q.astype(_f16).astype(_f32)
    k32, v32 = k.astype(_f32), v.astype(_f32)

    def scores(kk):
        part = np.zeros((B, Hh, S, 8), _f32)                               # lane (key, c)
        qc, kc = qv.reshape(B, Hh, 1, 8, 8), kk.reshape(B, Hh, S, 8, 8)
        for e in range(8):
            part = _fma(np.broadcast_to(qc[..., e], part.shape), kc[..., e], part)
        return part

    s = scores(k32)
    if mutation == "group_neighbour_head":                                  # the 8-key group at key0 = 8 reads K of head h + 1
        s[:, :, 8:16] = scores(np.roll(k32, -1, axis=1))[:, :, 8:16]
    if lo:
        s = (s + scores(k_lo.astype(_f32))).astype(_f32)
    s = _xor_sum(s)[..., 0]
    thr = lens + 1 if mutation == "mask_len_plus_1" else lens - 1 if mutation == "mask_len_minus_1" else lens
    s = (s + np.where(np.arange(S)[None, :] >= thr[:, None], _f32(-10000.0), _f32(0.0))[:, None, :]).astype(_f32)
    mx = s.max(-1, keepdims=True)
    p = np.exp((s - mx).astype(_f32)).astype(_f32)
    pr = p if lo else p.astype(_f16).astype(_f32)
    src = pr if mutation == "rounded_sum" else p
    lane_sum = np.zeros((B, Hh, 64), _f32)
    for j in range(S // 64):
        lane_sum = (lane_sum + src[..., 64 * j:64 * (j + 1)]).astype(_f32)
    inv = (_f32(1.0) / _xor_sum(lane_sum)[..., :1]).astype(_f32)
    drop = int((lens.min() - 1) // 64) if mutation == "pv_block_dropped" else -1   # a block that holds real keys of every sequence

    def pv(vv):
        acc = np.zeros((B, Hh, D, 8), _f32)                                 # lane (dim, c): keys kb0 + 8 c .. + 7
        for j in range(S // 64):
            if j == drop:
                continue
            pb = pr[..., 64 * j:64 * (j + 1)].reshape(B, Hh, 1, 8, 8)
            vb = vv[:, :, 64 * j:64 * (j + 1)].transpose(0, 1, 3, 2).reshape(B, Hh, D, 8, 8)
            for e in range(8):
                acc = _fma(np.broadcast_to(pb[..., e], acc.shape), vb[..., e], acc)
        return acc

    acc = pv(v32)
    if lo:
        acc = (acc + pv(v_lo.astype(_f32))).astype(_f32)
    out = _xor_sum(acc)[..., 0]
    if vlo_sp is not None and mutation != "vlo_sp_omitted":
        l2 = vlo_sp.astype(_f32)
        inner = _fma(np.broadcast_to(pr[..., 0:1], out.shape), l2[..., 0], (pr[..., 1:2] * l2[..., 1]).astype(_f32))
        out = _fma(inner, np.full(out.shape, 2.0 ** -10 if mutation == "vlo_sp_2_10" else 2.0 ** -11, _f32), out)
    out = (out * inv).astype(_f32)
    return out.astype(_f16).astype(_f32) if ctx16 else out


def emulate_dense768(x, W, bias, act, res=None, mutation=None):
    """dense768_kernel<act, KT>: 8 waves x KT / 8 ascending k (one fp32 accumulation per k), the partial tiles added in wave order, + bias, the activation,
    + the residual.  x [B, KT], W [N, KT], bias [N] fp32.  Returns [B, N] fp32."""
    assert mutation is None or mutation in DENSE_MUTATIONS
    B, KT = x.shape
    N = W.shape[0]
    KW = KT // 8
    x, W = x.astype(_f32), W.astype(_f32)
    rows = np.arange(B)
    if mutation == "clamped_row_stored" and B >= 2:                         # the clamp one row early: the last real row stores what row B - 2 computed
        rows = np.minimum(rows, B - 2)
    xs = x[rows]
    WT = np.ascontiguousarray(W.T)
    total = None
    for wv in range(8):
        acc = np.zeros((B, N), _f32)
        for kk in range(wv * KW, (wv + 1) * KW):
            if mutation == "chunk_dropped" and wv == 5 and 96 <= kk - wv * KW < 192:   # the second 96-chunk of wave 5
                continue
            acc = (acc.astype(_f64) + xs[:, kk:kk + 1].astype(_f64) * WT[kk][None, :].astype(_f64)).astype(_f32)
        if mutation == "wave_dropped" and wv == 3:
            acc[:] = 0
        total = acc if total is None else (total + acc).astype(_f32)
    b = bias.astype(_f32)
    if mutation == "bias_n_plus_32":
        b = np.roll(b, -32)
    v = (total + b[None, :]).astype(_f32)
    if act == ACT_TANH:
        v = np.tanh(v.astype(_f64)).astype(_f32)
    elif act == ACT_RELU:
        v = np.maximum(v, _f32(0))
    elif act == ACT_GELU:
        v = gelu64(v.astype(_f64)).astype(_f32)
    elif act == ACT_RES and mutation != "residual_omitted":
        v = (v + res.astype(_f32)).astype(_f32)
    return v


def emulate_gather(hi, lo, lo_scale, vst, g, b, Sp, mutation=None):
    """cls_gather_kernel's big path for B sequences: hi [B Sp, 768] fp16 (the stream's hi plane), lo the low parts — compact [2 B, 768] (MV_F16X8: sp_lo, row
    2 b, lo_scale 2^-11) or per token [B Sp, 768] (MV_F16: xlo, lo_scale 1) — vst [B Sp, 3, 2] fp32.  Returns (c32 fp32, c16 fp16) [B, 768]."""
    assert mutation is None or mutation in GATHER_MUTATIONS
    B = hi.shape[0] // Sp
    compact = lo.shape[0] == 2 * B
    t = np.arange(B) * Sp + (1 if mutation == "row_plus_1" else 0)
    lo_rows = (2 * np.arange(B) + (1 if mutation == "row_plus_1" else 0)) if compact else t
    scale = _f32(1.0 if mutation == "sp_lo_unscaled" else lo_scale)
    st = vst[t + (1 if mutation == "neighbour_stats" else 0)].astype(_f32)
    s1 = ((st[:, 0, 0] + st[:, 1, 0]).astype(_f32) + st[:, 2, 0]).astype(_f32)
    s2 = ((st[:, 0, 1] + st[:, 1, 1]).astype(_f32) + st[:, 2, 1]).astype(_f32)
    inv_h = _f32(1.0) / _f32(H)
    mean = (s1 * inv_h).astype(_f32)
    var = np.maximum(((s2 * inv_h).astype(_f32) - (mean * mean).astype(_f32)).astype(_f32), _f32(0))
    rstd = (1.0 / np.sqrt((var + _f32(LN_EPS)).astype(_f32).astype(_f64))).astype(_f32)
    y = _fma(lo[lo_rows].astype(_f32), np.full((B, H), scale, _f32), hi[t].astype(_f32))
    tt = (((y - mean[:, None]).astype(_f32)) * rstd[:, None]).astype(_f32)
    c32 = _fma(tt, np.broadcast_to(g.astype(_f32), tt.shape), np.broadcast_to(b.astype(_f32), tt.shape))
    return c32, c32.astype(_f16)


def emulate_ln(x, g, b):
    """ln_kernel<true> (misc_kernels.h ln_row_store) on rows x [B, 768] fp32: lane sums ((x + y) + (z + w), three float4 per lane), the butterfly, the centred
    variance by fma, 1 / sqrtf.  Returns (fp32, fp16)."""
    B = x.shape[0]
    x = x.astype(_f32)
    xl = x.reshape(B, 3, 64, 4)                                             # column 4 lane + 256 i
    s = np.zeros((B, 64), _f32)
    for i in range(3):
        s = (s + ((xl[:, i, :, 0] + xl[:, i, :, 1]).astype(_f32) + (xl[:, i, :, 2] + xl[:, i, :, 3]).astype(_f32)).astype(_f32)).astype(_f32)
    mean = (_xor_sum(s)[:, :1] * (_f32(1.0) / _f32(H))).astype(_f32)
    vv = np.zeros((B, 64), _f32)
    for i in range(3):
        for e in range(4):
            a = (xl[:, i, :, e] - mean).astype(_f32)
            vv = _fma(a, a, vv)
    var = ((_xor_sum(vv)[:, :1] * (_f32(1.0) / _f32(H))).astype(_f32) + _f32(LN_EPS)).astype(_f32)
    rstd = (_f32(1.0) / np.sqrt(var).astype(_f32)).astype(_f32)
    t = ((x - mean).astype(_f32) * rstd).astype(_f32)
    out = _fma(t, np.broadcast_to(g.astype(_f32), t.shape), np.broadcast_to(b.astype(_f32), t.shape))
    return out, out.astype(_f16)


# ---- the share of a bound an output uses -----------------------------------------------------------------------------------------------------------------------------

def share(got, ref, bound):
    """|got - ref| / bound per element (0 / 0 = 0: an exact stage with a zero bound)."""
    err = np.abs(np.asarray(got, _f64) - ref)
    b = np.broadcast_to(np.asarray(bound, _f64), err.shape)
    return np.where(err == 0.0, 0.0, err / np.where(b > 0.0, b, np.finfo(_f64).tiny))


def stats(r):
    return float(r.max()), float(np.sqrt((r ** 2).mean()))


# ---- a whole tail on an engine's taps ------------------------------------------------------------------------------------------------------------------------------------

def heads(x):
    """[B, 768] -> [B, 12, 64]."""
    return x.reshape(x.shape[0], HEADS, HD)


def check_tail(taps, tw, kind, big, lens, proj):
    """Every launch of one tapped tail against its model.  taps: float64 arrays by name — the tail's inputs (gather: `hi`, `lo` [B, 768] of the [CLS] rows, `vst`
    [B, 3, 2] on the big path, `x32`, `x16` on the small one; attention: `k`, `v` [B, 12, S, 64] (hi + lo already summed in the safe form), `vlo_sp`
    [B, 12, 64, 2] or None, `sp_keys`) and what the launches wrote (`g32`, `g16`, `q`, `ctx`, `out`, `ln1_32`, `ln1_16`, `ffn1`, `ffn2`, `ln2`, `pooled`, `u`).
    kind "precise" | "safe" | "f16".  Returns {launch: share array} — every real row and column; the exact stages (c16, ch16, a copy) are 0 or inf."""
    x8 = kind != "f16"
    r = {}
    if big:
        m, bnd = gather_model(taps["hi"], taps["lo"], 2.0 ** -11 if x8 else 1.0, taps["vst"], tw["pend_g"], tw["pend_b"])
        r["gather"] = share(taps["g32"], m, bnd)
        r["gather_c16"] = share(taps["g16"], f16(taps["g32"]), 0.0)
    else:
        r["gather"] = share(taps["g32"], taps["x32"], 0.0)
        r["gather_c16"] = share(taps["g16"], taps["x16"], 0.0)
    if x8:
        m, bnd, _ = dense_model(taps["g32"], tw["wq"], tw["bq"], ACT_ID)
    else:
        m, bnd = skinny_model(taps["g16"], tw["wq"], tw["bq"], "f32")
    r["q"] = share(taps["q"], m, bnd)
    q = heads(taps["q"])
    if kind == "safe":
        m, bnd = attn_safe_model(q, taps["k"], taps["v"], lens)
    elif kind == "precise":
        m, bnd = attn_exact_model(q, taps["k"], taps["v"], lens, taps.get("vlo_sp"), taps.get("sp_keys"))
    else:
        m, bnd = attn_f16_model(q, taps["k"], taps["v"], lens)
    r["attention"] = share(heads(taps["ctx"]), m, bnd)
    if x8:
        m, bnd, _ = dense_model(taps["ctx"], tw["wo"], tw["bo"], ACT_RES, taps["g32"])
    else:
        m, bnd = skinny_model(taps["ctx"], tw["wo"], tw["bo"], "res", taps["g32"])
    r["out_proj"] = share(taps["out"], m, bnd)
    m, bnd = ln_model(taps["out"], tw["ln1g"], tw["ln1b"])
    r["ln1"] = share(taps["ln1_32"], m, bnd)
    r["ln1_c16"] = share(taps["ln1_16"], f16(taps["ln1_32"]), 0.0)
    if x8:
        m, bnd, _ = dense_model(taps["ln1_32"], tw["w1"], tw["b1"], ACT_GELU)
    else:
        m, bnd = skinny_model(taps["ln1_16"], tw["w1"], tw["b1"], "gelu")
    r["ffn1"] = share(taps["ffn1"], m, bnd)
    if x8:
        m, bnd, _ = dense_model(taps["ffn1"], tw["w2"], tw["b2"], ACT_RES, taps["ln1_32"])
    else:
        m, bnd = skinny_model(taps["ffn1"], tw["w2"], tw["b2"], "res", taps["ln1_32"])
    r["ffn2"] = share(taps["ffn2"], m, bnd)
    m, bnd = ln_model(taps["ffn2"], tw["ln2g"], tw["ln2b"])
    r["ln2"] = share(taps["ln2"], m, bnd)
    m, bnd, _ = dense_model(taps["ln2"], tw["wp"], tw["bp"], ACT_TANH)
    r["pooler"] = share(taps["pooled"], m, bnd)
    if proj == PROJ:
        m, bnd, _ = dense_model(taps["pooled"], tw["wh"], tw["bh"], ACT_RELU)
        r["header"] = share(taps["u"], m, bnd)
    else:
        r["header"] = share(taps["u"], taps["pooled"], 0.0)               # use_header = False: the pooler writes u itself
    return r


def read_tail_taps(eng, kind, big, lens):
    """After eng.tail_encode(ids, lens): the operands and outputs check_tail wants, as float64, from the tail taps 22 - 33 and the taps of the tail's inputs."""
    f = lambda i: eng.debug_read(i).astype(_f64)  # noqa: E731
    B = len(lens)
    x8 = kind != "f16"
    t = dict(g32=f(22), g16=f(23), q=f(24), ctx=f(25), out=f(26), ln1_32=f(27), ln1_16=f(28), ffn1=f(29), ffn2=f(30), ln2=f(31), pooled=f(32), u=f(33))
    if big:
        t["hi"] = f(1)[:, 0]
        t["vst"] = f(13)[:, 0]
        t["lo"] = f(12).reshape(B, 2, H)[:, 0] if x8 else f(19)[:, 0]
    else:
        t["x32"], t["x16"] = f(0)[:, 0], f(1)[:, 0]
    Sp = eng._dbg[1]
    k, v = f(3)[:, :, :Sp], f(4)[:, :, :, :Sp].transpose(0, 1, 3, 2)
    if kind == "safe":
        k, v = k + f(8)[:, :, :Sp], v + f(9)[:, :, :, :Sp].transpose(0, 1, 3, 2)
    t["k"], t["v"] = k, v
    if kind == "precise" and Sp > 128:  # (encoder_pass.h special_v_lo: a pass of <= 128 keys is a two-plane pass and hands the tail no vlo_sp)
        t["vlo_sp"], t["sp_keys"] = f(18), gsk.special_rows(lens)
    return t
