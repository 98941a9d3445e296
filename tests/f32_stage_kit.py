"""Shared pieces of the reference-form stage tests (tests/test_f32_stage_cpu.py, tests/test_f32_stage_gpu.py): every launch of an MV_F32 pass
(encoder_pass.h encode_f32_dev: gemm_f32_kernel x 4, attention_f32_kernel, ln_kernel<true> x 2 per layer) against a float64 model formed from THAT LAUNCH'S OWN
operands — mv_debug_read 0, 35, 36, 37 of engines the development build's MEMVUL_DEBUG_STOP ended inside the layer — never from the previous model's output.
Plain module: no fixtures, no GPU.

GEMMs       |C - C64| <= 2 g(K) (|A| |W|^T + |bias| + |res|), g = 1.5e-7 at K = 768 and 3.5e-7 at K = 3072 — the fmaf chain's measured constants, the bound
            tests/test_f32_form_gpu.py test_gemm_against_float64 holds on caller data (gemm_g, gemm_bound: that test imports them from here).  GELU: 1.13 x
            that (its Lipschitz constant) + 4 fp32 roundings of the result.
LayerNorm   cls_tail_kit.ln_model: the roundings ln_kernel<true> performs, derived.
Attention   per query row < len, head and dim:   bound = pav x (C_S x u x smag + 8 u)
              u     2^-24
              pav   sum_k p_k |v_k|                      (stage_kit.attention_terms64)
              smag  max_k sum_d |q_d k_d| of the query   (smag64)
            What moves a context element in fp32 is the error of the exponent's ARGUMENT: a score is a chain of 64 products, its rounding error scales with
            sum_d |q_d k_d| (not with the score, which cancels), and exp turns an absolute error e of s - max into a relative error e of p.  So the first term is
            (chain constant) x u x smag, relative to pav.  The second: p = exp(.) x inv (2 roundings), the row sum behind inv (each p's own rounding averages
            out; the chunk combine and the rescale add 3 per chunk, relative to l), 1 / l (1) and the P V chain, whose k-th partial sum is bounded by pav itself —
            8 u covers what the emulation shows of them at the low-spread end of the table, where the first term is small (C_S was measured WITHOUT the 8 u: the
            8 u is slack at small spread, not part of the constant).
            The worst-case chain constant (64 products + 64 sums: 128 u) is useless: 60 - 100 x above what fp32 does, and above the error of a 16-bit alias once
            scores spread beyond about 4.  C_S is a MEASURED chain constant, as the GEMM's g(K) is — measured on the numpy emulation below (emulate_attention_f32:
            the kernel's own order, fp32, FMA-exact), never on the kernel:
              C_S = 2 x max over CS_TABLE of |ctx_emulated - ctx64| / (pav x u x smag)
            tests/test_f32_stage_cpu.py recomputes the maximum (test_the_chain_constant_is_the_measured_one) and fails when 2 x it leaves [0.9, 1.0] x C_S:
            measured 2.932 (padded length 128, score std 20), so C_S = 5.9.  By case of the table the maximum reads 0.95 - 1.88 at std 1, 1.80 - 2.80 at std 4,
            2.16 - 2.64 at std 10 and 2.08 - 2.93 at std 20: it hardly moves with the spread or the length, which is what makes it a constant.
            The factor 2: the emulation follows the kernel's order but neither the device expf (about 1 ulp of its own, where numpy's float32 exp is
            correctly rounded to within an ulp as well but not the same function) nor what v_mfma_f32_32x32x2_f32 does between its two products; and the
            engine's operands are not the table's Gaussians.  With it the unmutated emulation stays <= 0.5 of the bound by construction.
            Query rows >= len need only be finite, and ALL of ctx32 has to be finite: pass 2 multiplies p = 0 into the V rows of the masked keys of the last chunk.
tests/test_f32_stage_cpu.py shows the faults the bound catches (MUTATIONS) in every case of the table where they can act."""
import numpy as np

import cls_tail_kit as ctk
import stage_kit as sk

H, INTER, HEADS, HD = 768, 3072, 12, 64
U = 2.0 ** -24
C_S = 5.9
_f32, _f16, _f64 = np.float32, np.float16, np.float64


# ---- GEMMs ---------------------------------------------------------------------------------------------------------------------------------------------------------

def gemm_g(K):
    """The fmaf chain's measured constant of gemm_f32_kernel at the engine's two K."""
    return 1.5e-7 if K == 768 else 3.5e-7


def gemm_bound(act, g, mag, want=None, res=None):
    """act "bias": 2 g mag; "gelu": 1.13 x that + 4 x 6e-8 |want|; "res": 2 g (mag + |res|).  mag = |A| |W|^T + |bias|."""
    if act == "bias":
        return 2 * g * mag
    if act == "gelu":
        return 1.13 * 2 * g * mag + 4 * 6e-8 * np.abs(want)
    return 2 * g * (mag + np.abs(res))


def gemm_model(A, W, bias, act, res=None):
    """(float64 model, bound) of act(A W^T + bias) (+ res): A [M, K], W [N, K], bias [N], res [M, N], all float64 holding fp32 values."""
    pre = A @ W.T + bias
    mag = np.abs(A) @ np.abs(W).T + np.abs(bias)
    g = gemm_g(A.shape[1])
    if act == "bias":
        return pre, gemm_bound("bias", g, mag)
    if act == "gelu":
        want = ctk.gelu64(pre)
        return want, gemm_bound("gelu", g, mag, want=want)
    return pre + res, gemm_bound("res", g, mag, res=res)


def layer_weights(w, l):
    """float64 matrices [N, K] of layer l (0-based) as weights.h stores them for MV_F32: the packed Q | K | V with 1 / 8 folded into the Q block and b_q (exact:
    a power of two), W_o, W_1, W_2 un-folded, the two LayerNorms."""
    from oracle import memvul_oracle as orc

    p = orc.PFX + f"encoder.layer.{l}."
    g = lambda k: np.asarray(w[k], _f32).astype(_f64)  # noqa: E731
    a = p + "attention.self."
    return dict(wqkv=np.concatenate([ctk.f32(g(a + "query.weight") * 0.125), g(a + "key.weight"), g(a + "value.weight")]),
                bqkv=np.concatenate([ctk.f32(g(a + "query.bias") * 0.125), g(a + "key.bias"), g(a + "value.bias")]),
                wo=g(p + "attention.output.dense.weight"), bo=g(p + "attention.output.dense.bias"),
                w1=g(p + "intermediate.dense.weight"), b1=g(p + "intermediate.dense.bias"),
                w2=g(p + "output.dense.weight"), b2=g(p + "output.dense.bias"),
                ln1g=g(p + "attention.output.LayerNorm.weight"), ln1b=g(p + "attention.output.LayerNorm.bias"),
                ln2g=g(p + "output.LayerNorm.weight"), ln2b=g(p + "output.LayerNorm.bias"))


# ---- attention -----------------------------------------------------------------------------------------------------------------------------------------------------

def split_qkv(qkv):
    """Tap 35 [B, Sp, 2304] -> q, k, v float64 [B, 12, Sp, 64]."""
    B, S, _ = qkv.shape
    x = np.asarray(qkv, _f64).reshape(B, S, 3, HEADS, HD).transpose(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads_of(ctx):
    """Tap 36 [B, Sp, 768] -> [B, 12, Sp, 64]."""
    B, S, _ = ctx.shape
    return np.asarray(ctx, _f64).reshape(B, S, HEADS, HD).transpose(0, 2, 1, 3)


def smag64(q, k, lens):
    """max over the sequence's own keys of sum_d |q_d k_d|, per query: [B, H, S, 1]."""
    out = np.zeros(q.shape[:3] + (1,))
    for b, n in enumerate(np.asarray(lens)):
        out[b, :, :, 0] = (np.abs(q[b]) @ np.abs(k[b, :, :int(n)]).transpose(0, 2, 1)).max(-1)
    return out


def attention_bound(t, smag, c_s=C_S):
    return t["pav"] * (c_s * U * smag + 8.0 * U)


def attention_share(ctx, q, k, v, lens, c_s=C_S):
    """|ctx - float64| / bound as [B, H, S, D] with the query rows >= len at 0 (NaN / inf in ctx on a real row -> inf), and the same with the 8 u term left out of
    the bound and C_S = 1: the chain constant the output shows."""
    t = sk.attention_terms64(q, k, v, lens)
    sm = smag64(q, k, lens)
    m = sk.row_mask(lens, ctx.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(ctx - t["ref"])
        share = np.where(m, err / attention_bound(t, sm, c_s), 0.0)
        chain = np.where(m, err / (t["pav"] * U * sm), 0.0)
    return np.where(np.isfinite(share), share, np.inf), np.where(np.isfinite(chain), chain, np.inf)


# ---- numpy emulation of attention_f32_kernel's arithmetic ------------------------------------------------------------------------------------------------------------

MUTATIONS = ("mask_len_plus_1", "mask_len_minus_1", "half_wave_max", "no_rescale", "key_map", "d_half", "p_fp16")
# the lanes of a wave hold the 32 keys of a chunk as 2 halves x 16 registers: register r of half hi = key mfma32_row(r, hi) (common.h)
_ROW = np.array([[(r & 3) + 8 * (r >> 2) + 4 * hi for r in range(16)] for hi in range(2)])


def emulate_scores(q, k):
    """S = Q K^T as attention_f32_kernel's `scores` forms it: 32 issues from zero, issue t adds (d = t, d = 32 + t) — two fp32 fused multiply-adds, lanes 0 - 31
    before lanes 32 - 63.  q, k fp32 [B, H, S, 64] -> fp32 [B, H, Sq, Sk], every key unmasked."""
    q, k = q.astype(_f32), k.astype(_f32)
    B, Hh, S, _ = q.shape
    s = np.zeros((B, Hh, S, S), _f32)
    for t in range(32):
        for d in (t, t + 32):
            s = ctk._fma(np.broadcast_to(q[..., :, None, d], s.shape), np.broadcast_to(k[..., None, :, d], s.shape), s)
    return s


def emulate_attention_f32(q, k, v, lens, mutation=None, scores=None):
    """attention_f32_kernel in its own order, fp32: per (sequence, head, query) chunks of 32 keys; pass 1 — per half-wave (16 keys) the maximum, combined across the
    halves, a = the sequential sum of exp(s - max) over the half's 16 registers, the halves added, l = fma(l, exp(m_old - m_new), a); pass 2 — p = exp(s - m) x
    (1 / l), normalised BEFORE the P V chain, which runs over the chunk's keys in the order the MFMA contracts them: issue r adds keys (kr, kr + 4),
    kr = (r & 3) + 8 (r >> 2).  Chunks past len are not visited; masked keys of the last chunk carry p = 0 times whatever V holds.  Every query row is computed.
    q, k, v fp32 [B, H, S, 64] (q carries the 1 / 8); scores: emulate_scores(q, k) if the caller has it.  Returns fp32 [B, H, S, 64].
    mutation: one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    B, Hh, S, D = q.shape
    v = v.astype(_f32)
    s_all = emulate_scores(q, k) if scores is None else scores
    out = np.zeros((B, Hh, S, D), _f32)
    for b in range(B):
        n = int(min(max(int(lens[b]), 1), S))
        if mutation == "mask_len_plus_1":
            n = min(n + 1, S)                                               # key `len` taken for a real one
        masked_from = max(n - 1, 1) if mutation == "mask_len_minus_1" else n  # (len 1: key 0 stays, as the kernel's clamp keeps it)
        nch = (n + 31) // 32
        with np.errstate(invalid="ignore", over="ignore"):

            def chunk(c):  # [H, Sq, 2, 16]: the chunk's scores per half and register, masked keys = -inf
                sc = s_all[b, :, :, 32 * c:32 * c + 32].copy()
                sc[..., np.arange(32 * c, 32 * c + 32) >= masked_from] = -np.inf
                return sc[..., _ROW]

            m = np.full((Hh, S, 2), -np.inf, _f32)
            l = np.zeros((Hh, S, 2), _f32)
            for c in range(nch):
                sh = chunk(c)
                cm = sh.max(-1)
                if mutation != "half_wave_max":
                    cm = np.broadcast_to(cm.max(-1, keepdims=True), cm.shape)
                mn = np.maximum(m, cm)
                a = np.zeros((Hh, S, 2), _f32)
                for r in range(16):
                    a = (a + np.exp((sh[..., r] - mn).astype(_f32)).astype(_f32)).astype(_f32)
                a = np.broadcast_to((a[..., 0] + a[..., 1]).astype(_f32)[..., None], a.shape)
                if mutation == "no_rescale":
                    l = (l + a).astype(_f32)
                else:
                    l = ctk._fma(l, np.exp((m - mn).astype(_f32)).astype(_f32), a)
                m = mn
            inv = (_f32(1.0) / l).astype(_f32)
            o = np.zeros((Hh, S, D), _f32)
            for c in range(nch):
                sh = chunk(c)
                p = (np.exp((sh - m[..., None]).astype(_f32)).astype(_f32) * inv[..., None]).astype(_f32)
                if mutation == "p_fp16":
                    p = p.astype(_f16).astype(_f32)
                for r in range(16):
                    for hi in range(2):
                        vkey = 32 * c + (r + 4 * hi if mutation == "key_map" else _ROW[hi, r])   # key_map: V of key r (+ 4) where the map says (r & 3) + 8 (r >> 2)
                        o = ctk._fma(np.broadcast_to(p[..., hi, r][..., None], o.shape), np.broadcast_to(v[b, :, vkey][:, None, :], o.shape), o)
        if mutation == "d_half":                                            # the `+ 32` of the second store lost: o1 lands on o0's columns
            out[b, :, :, :32] = o[..., 32:]
        else:
            out[b] = o
    return out


# ---- the case table C_S is measured on -------------------------------------------------------------------------------------------------------------------------------
# (padded length, lens): every len of {1, 2, 31, 32, 33, 63, 64, 65, 97, 225, 385, 512}, each at the smallest padded length that holds it, and the full ones
CS_BATCHES = ((64, (1, 2, 31, 32, 33, 63, 64)), (128, (65, 97, 128)), (256, (225, 256)), (512, (385, 512)))
CS_STDS = (1.0, 4.0, 10.0, 20.0)
CS_TABLE = tuple((Sp, lens, std) for Sp, lens in CS_BATCHES for std in CS_STDS)
CS_HEADS = {64: 4, 128: 2, 256: 2, 512: 1}  # (heads drawn per padded length: 100+ real queries per sequence from len 31 on, and a table that runs in seconds)


def table_operands(Sp, lens, std):
    """fp32 Q, K, V [B, CS_HEADS[Sp], Sp, 64] whose scores have standard deviation `std`; the rows past len hold finite values like any other (the engine's do)."""
    rng = np.random.default_rng(int(1000 * Sp + 10 * std + len(lens)))
    a = np.sqrt(std / np.sqrt(HD))
    return tuple((rng.standard_normal((len(lens), CS_HEADS[Sp], Sp, HD)) * sc).astype(_f32) for sc in (a, a, 1.0))


def can_act(mutation, n, Sp):
    """Whether the fault changes anything for a sequence of n tokens at padded length Sp; the cases where it cannot are the exemptions the CPU test lists."""
    if mutation == "mask_len_plus_1":
        return n < Sp                      # there is no key `len`
    if mutation == "mask_len_minus_1":
        return n >= 2                      # the kernel clamps len to 1: key 0 stays
    if mutation == "no_rescale":
        return n > 32                      # one chunk: nothing to rescale
    if mutation == "key_map":
        return n > 8                       # registers 0 - 3 map to keys 0 - 7 either way; every other key's p is 0
    if mutation == "half_wave_max":
        return n >= 2                      # one key: len 1 is exempt with the issue's list (the half without a key then holds -inf - -inf)
    if mutation == "p_fp16":
        return n >= 2                      # one key: p = 1, an fp16 number
    return True
