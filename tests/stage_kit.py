"""Shared pieces of the stage-parity tests (tests/test_stage_parity_gpu.py, tests/test_stage_parity_cpu.py, tests/test_safe_form_gpu.py): the float64 attention
the engine's own Q / K / V planes go through, the per-element bounds derived from the roundings attention_v2_kernel performs, the boundary batches, and a numpy
emulation of the kernel's arithmetic with the faults the bounds have to catch.  Plain module: no fixtures, no GPU."""
import numpy as np

HEADS, HEAD_DIM = 12, 64


def host_source():
    """The host source of the library as one text, for the tests that read it: engine.hip, then the parts it includes, in include order — taken from
    build.SOURCES and build.HEADERS (a part engine.hip includes but the build does not list, or in another order, fails here)."""
    import os
    import re

    from memvul_amd import build

    texts = [open(os.path.join(build.CSRC, s)).read() for s in build.SOURCES]
    included = [i for t in texts for i in re.findall(r'^#include "([^"/]+)"', t, flags=re.M)]
    assert included == [h for h in build.HEADERS if not os.path.isabs(h)] == build.KERNEL_HEADERS + build.HOST_PARTS, included
    return "\n".join(texts + [open(os.path.join(build.CSRC, p)).read() for p in build.HOST_PARTS])

# ---- the passes --------------------------------------------------------------------------------------------------------------------------------------------------
# (padded length, input width, the lengths of the rows): one batch per padded length, its rows ON the edges of the key mask (thr = len - j S - 8 hi: every
# 8-key half, 16-key k-slot group, 32-key fragment, 64-key block and 128-key chunk from both sides), of the chunk hand-over (a chunk wholly past len still
# rescales O) and of the padded widths (an input narrower than its padded length)
BOUNDARY_BATCHES = (
    (64, 64, (1, 2, 3, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)),
    (128, 128, (1, 2, 16, 63, 64, 65, 96, 127, 128)),
    (192, 192, (1, 2, 64, 65, 128, 129, 191, 192)),
    (192, 130, (129, 130)),
    (256, 256, (1, 3, 127, 128, 129, 192, 193, 255, 256)),
    (384, 384, (1, 2, 127, 128, 129, 255, 256, 257, 383, 384)),
    (384, 320, (1, 129, 257, 319, 320)),
    (512, 512, (1, 2, 8, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512)),
)
# tests/test_gpu_kernels.py test_attention_persistent_item_loop: more units than resident workgroups, neighbouring units of different lengths
ITEM_LOOP_SHAPES = ((48, 256), (70, 128), (40, 192), (26, 512), (30, 384), (21, 320))


def padded_len(S):
    """encoder_pass.h padded_len: 64 .. 256 in steps of 64, then 384, 512."""
    return (S + 63) // 64 * 64 if S <= 256 else (S + 127) // 128 * 128


def batch_id(batch):
    return "p%d_w%d" % (batch[0], batch[1])


def boundary_ids(width, lens, vocab_size, seed=0):
    """ids int32 [len(lens), width] with exactly these row lengths (synth.make_ids draws its ragged lengths itself): random ordinary tokens, [CLS] first, [SEP]
    last, 0 past the end."""
    lens = np.asarray(lens, np.int32)
    assert lens.min() >= 1 and lens.max() <= width
    rng = np.random.default_rng(1000 * width + seed)
    ids = rng.integers(min(1000, max(3, vocab_size // 2)), vocab_size, size=(len(lens), width)).astype(np.int32)
    cls_id, sep_id = (101, 102) if vocab_size > 102 else (1, 2)
    for b, n in enumerate(lens):
        ids[b, 0] = cls_id
        ids[b, n - 1] = sep_id
        ids[b, n:] = 0
    return ids, lens


def two_plane(engine, Sp):
    """The pass carries Q, K, V, P as hi + lo fp16 planes (encoder_pass.h two_plane_pass): the safe form at every padded length, the default form of MV_F16X8 up to
    128; MV_F16 never."""
    return engine == "safe" or (engine == "precise" and Sp <= 128)


def chunk_keys(Sp, planes2):
    """Keys per chunk of the online softmax (encoder_pass.h ATTN_VARIANTS, the table launch_attention reads): one-plane passes hold the whole key range up to 256 and walk chunks of 128 at 384 / 512;
    the two-plane ring holds it up to 128, walks chunks of 64 at 192 and of 128 above."""
    if planes2:
        return Sp if Sp <= 128 else 64 if Sp == 192 else 128
    return Sp if Sp <= 256 else 128


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------------------------------

def attention64(q, k, v, lens, round_p):
    """softmax(q k^T + additive mask) v in float64 per (row, head): q, k [B, 12, S, 64] (q carries the folded 1 / 8), v [B, 12, S, 64].  round_p: the
    un-normalised probabilities exp(s - max) rounded to fp16 in the numerator, the row sum from the unrounded ones (what a one-plane kernel computes)."""
    B, H, S, D = q.shape
    s = np.einsum("bhqd,bhkd->bhqk", q, k)
    s = s + np.where(np.arange(S)[None, :] < np.asarray(lens)[:, None], 0.0, -10000.0)[:, None, None, :]
    p = np.exp(s - s.max(-1, keepdims=True))
    num = p.astype(np.float16).astype(np.float64) if round_p else p
    return np.einsum("bhqk,bhkd->bhqd", num, v) / p.sum(-1, keepdims=True)


def attention_terms64(q, k, v, lens):
    """The same attention (P unrounded) and what the bounds are made of, for the query rows < len of every sequence (the other rows stay 0):
      ref   softmax(q k^T + additive -10000 mask) v
      pav   sum_k p_k |v_k|
      sp    p_0 |v_0| + p_sep |v_sep|, sep = the sequence's last token (len >= 3; token 1 below that: the row the engine's special-row V term reads as key 1)
      vmax  max |v| over the sequence's own keys, per (row, head): [B, H, 1, 1]
    q, k, v float64 [B, H, S, D]."""
    B, H, S, D = q.shape
    lens = np.asarray(lens)
    ref, pav, sp = np.zeros(q.shape), np.zeros(q.shape), np.zeros(q.shape)
    vmax = np.zeros((B, H, 1, 1))
    av = np.abs(v)
    for b in range(B):
        n = int(lens[b])
        s = q[b, :, :n] @ k[b].transpose(0, 2, 1)                      # [H, n, S]: every key of the padded row, masked as the reference masks
        s = s + np.where(np.arange(S) < n, 0.0, -10000.0)[None, None, :]
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        ref[b, :, :n] = p @ v[b]
        pav[b, :, :n] = p @ av[b]
        sep = n - 1 if n >= 3 else 1
        sp[b, :, :n] = p[:, :, 0:1] * av[b, :, None, 0]
        if sep < S:
            sp[b, :, :n] += p[:, :, sep:sep + 1] * av[b, :, None, sep]
        vmax[b, :, 0, 0] = av[b, :, :n].max(axis=(1, 2))
    return dict(ref=ref, pav=pav, sp=sp, vmax=vmax)


def row_mask(lens, shape):
    """bool [B, H, S, D]: the query rows < len."""
    B, H, S, D = shape
    return np.broadcast_to((np.arange(S)[None, :] < np.asarray(lens)[:, None])[:, None, :, None], shape)


# ---- the bounds: derived from the roundings the kernel performs, not measured -------------------------------------------------------------------------------------

def bound_two_plane(t):
    """Q, K, V, P as hi + lo: what is left is the fp16 store of O (2^-11 |ref|) and, with a factor 2, fp32 accumulation over at most 512 products (512 x 2^-24 =
    2^-15), the fp32 exponent argument and the dropped lo x lo terms (2^-22) — 2^-14 max |V| per head (tests/test_safe_form_gpu.py)."""
    return 2.0 ** -11 * np.abs(t["ref"]) + 2.0 ** -14 * t["vmax"]


def bound_one_plane(t, special_rows=False):
    """One plane: + the worst-case fp16 rounding of P, 2^-11 sum_k p_k |v_k| (every p_k half an ulp off in the direction of sign(v_k); a model that rounds P
    itself would have to follow the kernel's per-chunk running maximum); 2^-14 max |V| covers fp32 accumulation, the hardware exp2 and subnormal P.
    special_rows (MV_F16X8 above 128 keys): the kernel adds the low parts of V of its keys 0 and 1 — the [CLS] and the last token — which no tap exposes and
    the reference therefore leaves out: + 2^-12 (p_0 |v_0| + p_sep |v_sep|)."""
    b = 2.0 ** -11 * np.abs(t["ref"]) + 2.0 ** -11 * t["pav"] + 2.0 ** -14 * t["vmax"]
    if special_rows:
        b = b + 2.0 ** -12 * t["sp"]
    return b


def bound_for(engine, Sp, t):
    if two_plane(engine, Sp):
        return bound_two_plane(t)
    return bound_one_plane(t, special_rows=(engine == "precise"))


def ratio_stats(ctx, t, bound, lens):
    """(max, rms) of |ctx - ref| / bound over every query row < len, every head, every dim."""
    m = row_mask(lens, ctx.shape)
    r = (np.abs(ctx - t["ref"]) / bound)[m]
    return float(r.max()), float(np.sqrt((r ** 2).mean()))


# ---- the engine's own operands ------------------------------------------------------------------------------------------------------------------------------------

def read_attention_taps(eng, S, planes2):
    """After debug_encode(ids, lens, n): the operands and the result of layer n's attention as float64 [B, 12, S, 64] — taps 2, 3, 4 (Q, K, V^T), their low planes
    7, 8, 9 added where the pass wrote them (planes2), and tap 5 (the context)."""
    f64 = lambda b: eng.debug_read(b).astype(np.float64)  # noqa: E731
    q, k, v = f64(2)[:, :, :S], f64(3)[:, :, :S], f64(4)[:, :, :, :S].transpose(0, 1, 3, 2)
    if planes2:
        q, k, v = q + f64(7)[:, :, :S], k + f64(8)[:, :, :S], v + f64(9)[:, :, :, :S].transpose(0, 1, 3, 2)
    ctx = f64(5)[:, :S]
    ctx = ctx.reshape(ctx.shape[0], S, HEADS, HEAD_DIM).transpose(0, 2, 1, 3)
    return q, k, v, ctx


def attention_ratio(eng, engine, ids, lens, n_layers):
    """Layer n_layers' attention of `eng` (an engine of kind `engine`: "precise" | "safe" | "f16") on its own operands: (max, rms) of |ctx - float64| / bound over
    every real row, head and dim."""
    eng.debug_encode(ids, lens, n_layers)
    S = ids.shape[1]
    Sp = padded_len(S)
    q, k, v, ctx = read_attention_taps(eng, S, two_plane(engine, Sp))
    assert np.isfinite(ctx[row_mask(lens, ctx.shape)]).all()
    t = attention_terms64(q, k, v, lens)
    return ratio_stats(ctx, t, bound_for(engine, Sp, t), lens)


# ---- numpy emulation of attention_v2_kernel's arithmetic ----------------------------------------------------------------------------------------------------------

MUTATIONS = ("unmasked_key", "no_rescale", "neighbour_rows", "v_swap")
_f32, _f16 = np.float32, np.float16
_LOG2E = np.float32(1.44269504088896340736)


def emulate_attention(q, k, v, lens, chunk, lo=None, mutation=None):
    """attention_v2_kernel step by step: fp32 scores (fp16 products, fp32 sums), the additive -10000 mask on keys >= len, per chunk of `chunk` keys the running
    maximum, p = exp2(fma(s, log2 e, -m log2 e)) in fp32, the row sum from the fp32 p, P rounded to fp16, O = O exp2((m_old - m_new) log2 e) + P V in fp32, and at
    the end fp16(O / l).  q, k, v fp16 [B, H, S, D] with S the padded length (q carries the 1 / 8); lo = (q_lo, k_lo, v_lo): the two-plane path (S^T += K_hi Q_lo
    + K_lo Q_hi, P_lo = fp16(p - fp16(p)), O += V_lo P_hi + V_hi P_lo).  Returns fp16 [B, H, S, D].
    mutation: one of MUTATIONS — key `len` left unmasked; the rescale of O skipped; the context of a work item written to its neighbour's rows; tokens 1 and
    len - 1 exchanged in V only (what a missed special-row permutation of one operand would be)."""
    assert mutation is None or mutation in MUTATIONS
    B, H, S, D = q.shape
    assert S % chunk == 0
    lens = np.asarray(lens)
    q32, k32, v32 = q.astype(_f32), k.astype(_f32), v.astype(_f32)
    vl32 = None
    if lo is not None:
        ql32, kl32, vl32 = (x.astype(_f32) for x in lo)
    if mutation == "v_swap":
        v32 = v32.copy()
        vl32 = None if vl32 is None else vl32.copy()
        for b, n in enumerate(lens):
            if n >= 3:
                for x in (v32, vl32):
                    if x is not None:
                        x[b, :, [1, n - 1]] = x[b, :, [n - 1, 1]]
    s = q32 @ k32.transpose(0, 1, 3, 2)
    if lo is not None:
        s = s + ql32 @ k32.transpose(0, 1, 3, 2)
        s = s + q32 @ kl32.transpose(0, 1, 3, 2)
    masked_from = lens + 1 if mutation == "unmasked_key" else lens
    s = s + np.where(np.arange(S)[None, :] < masked_from[:, None], _f32(0), _f32(-10000.0)).astype(_f32)[:, None, None, :]
    o = np.zeros((B, H, S, D), _f32)
    m_run = l_run = None
    for j in range(S // chunk):
        ks = slice(j * chunk, (j + 1) * chunk)
        sc = s[..., ks]
        mx = sc.max(-1, keepdims=True)
        alpha = None
        if j > 0:
            m_new = np.maximum(m_run, mx)
            alpha = np.exp2((m_run - m_new) * _LOG2E)
            mx = m_new
        m_run = mx
        nm = -mx * _LOG2E
        p = np.exp2((sc.astype(np.float64) * np.float64(_LOG2E) + nm.astype(np.float64)).astype(_f32))  # (one rounding: the fma)
        psum = p.sum(-1, keepdims=True, dtype=_f32)
        l_run = psum if j == 0 else l_run * alpha + psum
        ph = p.astype(_f16).astype(_f32)
        pv = ph @ v32[:, :, ks]
        if lo is not None:
            pl = (p - ph).astype(_f16).astype(_f32)
            pv = pv + ph @ vl32[:, :, ks] + pl @ v32[:, :, ks]
        if j > 0 and mutation != "no_rescale":
            o = o * alpha
        o = o + pv
    out = (o * (_f32(1.0) / l_run)).astype(_f16)
    if mutation == "neighbour_rows":  # the O tile of item (row, head) lands where the NEXT item of the work list writes
        out = np.roll(out.reshape(B * H, S, D), 1, axis=0).reshape(B, H, S, D)
    return out


def random_operands(B, H, S, lens, score_std, seed, planes2):
    """fp16 Q, K, V [B, H, S, D] (and their lo planes) whose scores have standard deviation `score_std`; rows past len hold finite values like any other (the
    engine's padded rows do: they are masked, not zeroed)."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(score_std / np.sqrt(HEAD_DIM))
    x = [rng.standard_normal((B, H, S, HEAD_DIM)) * sc for sc in (a, a, 1.0)]
    hi = [t.astype(_f16) for t in x]
    lo = [(t - h.astype(np.float64)).astype(_f16) for t, h in zip(x, hi)] if planes2 else None
    return hi, lo


def emulation_ratio(Sp, lens, score_std, seed, planes2, mutation=None, H=2):
    """|emulation - float64| / bound per element over the real rows: the emulation (with `mutation`) on random operands at padded length Sp, the reference and the
    bound exactly as attention_ratio builds them from the engine's taps.  Returns the ratios as [B, H, S, D] with the other rows at 0."""
    lens = np.asarray(lens)
    hi, lo = random_operands(len(lens), H, Sp, lens, score_std, seed, planes2)
    out = emulate_attention(*hi, lens, chunk_keys(Sp, planes2), lo=lo, mutation=mutation).astype(np.float64)
    f = [t.astype(np.float64) for t in hi]
    if planes2:
        f = [a + b.astype(np.float64) for a, b in zip(f, lo)]
    t = attention_terms64(*f, lens)
    bound = bound_two_plane(t) if planes2 else bound_one_plane(t)
    return np.where(row_mask(lens, out.shape), np.abs(out - t["ref"]) / bound, 0.0)
