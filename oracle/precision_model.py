"""CPU ORACLE (test infrastructure — NOT the product path): a float64 model of WHERE the HIP engine rounds.

The engine (memvul_amd/csrc) computes the reference's BERT forward (custom_PTM_embedder.py:228, HF BertModel) with
fp16 MFMA operands and fp32 accumulation.  This module re-runs the oracle's mathematics in float64 and applies a
rounding function at exactly the tensors the engine rounds:

  ``w_qkv, w_o, w_1, w_2``   the four weight matrices of a layer (QKV / FFN-1 after LayerNorm folding)
  ``a_qkv, a_ffn1``          the raw residual stream as the A operand of the QKV / FFN-1 GEMM (the ``hi`` plane)
  ``qkv``                    Q, K, V^T as stored between the projection and the attention kernel
  ``p``                      softmax probabilities as the A operand of P·V
  ``ctx``                    attention context (A operand of the output projection)
  ``h``                      GELU output (A operand of FFN-2)
  ``res``                    the raw residual stream AS STORED between the residual GEMMs (what the next residual add and its
                             LayerNorm read back; the row statistics are taken from the fp32 accumulators before the store):
                             "f16x2" = hi + lo fp16 planes (rounds 1-4), "f16x8" = hi fp16 + the lo8 plane of MV_F16X8 (round 5)

Each knob is a per-layer list of formats: ``"f16"``, ``"f16x2"`` (hi + lo split, 22 bits), ``"bf16"``, ``"bf16x2"``,
``"bf16x3"``, ``"exact"``, ``"f16x8"`` (the MV_F16X8 planes; as an A-operand format ``"f16x8w"`` = only the weight-side term swept,
``"f16x8q"`` / ``k`` / ``v`` = the A-side term only in that block of the packed QKV projection).  ``logit_error_table`` prints what each rounding point costs on the match logits, so a
precision change to the engine is chosen by measurement before any kernel is touched (tests/test_precision_model.py).
Everything else (LayerNorm statistics, softmax, residual adds, pooler, header, matcher) is fp32/fp64-exact here, as
in the engine (fp32).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from . import memvul_oracle as orc

PFX = orc.PFX


def _f16(x):
    return x.astype(np.float16).astype(np.float64)


def _bf16(x):
    """round-to-nearest-even to 8 significand bits (bfloat16), via the float32 bit pattern."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _e4m3(x):
    """round-to-nearest-even to OCP e4m3fn (4 significant bits, normal range 2^-6 .. 448, subnormal step 2^-9), saturating —
    what ``v_cvt_pk_fp8_f32`` after a clamp to +-448 produces on gfx950."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    e = np.clip(np.frexp(a)[1] - 1, -6, 8)  # a = m 2^e', m in [0.5, 1): binade floor(log2 a) = e' - 1 (zero: e' = 0, clipped like any tiny value)
    q = np.ldexp(1.0, e - 3)
    return np.copysign(np.minimum(np.rint(a / q) * q, 448.0), x)


# static power-of-two pre-scales of the fp8 planes (engine: MV_F16X8; the E8M0 scale operands of the MX instruction undo them
# exactly): activations 2^2 (|x| up to 112 representable), weights per matrix from max |W|
X8_ACT_SHIFT = 2


def _x8_planes(x, shift):
    """hi = fp16(x); hi8 = e4m3(hi 2^shift); lo8 = e4m3((x - hi) 2^(11 + shift)), returned de-scaled."""
    hi = _f16(x)
    s = 2.0 ** shift
    return hi, _e4m3(hi * s) / s, _e4m3((x - hi) * (2048.0 * s)) / (2048.0 * s)


def _w_shift(w):
    m = float(np.abs(w).max())
    return int(np.floor(np.log2(448.0 / m))) if m > 0 else 0


_W_PLANES = {}  # planes of WEIGHT operands: the same 48 matrices meet every evaluation of a test module (float32 holds them exactly)


def _w_planes(W):
    key = (W.shape, float(W[0, 0]), float(W[-1, -1]), float(W[W.shape[0] // 2, W.shape[1] // 3]), float(W.sum()))
    hit = _W_PLANES.get(key)
    if hit is None:
        if len(_W_PLANES) >= 64:
            _W_PLANES.clear()
        hit = tuple(p.astype(np.float32) for p in _x8_planes(W, _w_shift(W)))
        _W_PLANES[key] = hit
    return tuple(p.astype(np.float64) for p in hit)


# Round 6, model only: alternative forms of the WEIGHT-SIDE term A_hi8 W_lo8^T (the 300 us per layer every row still pays).
#   None       e4m3 x e4m3, every K-tile (the engine)
#   "fp4"      both operands as MX-fp4 (e2m1, one power-of-two scale per 32 K-elements): 4x the fp16 matrix rate, half the bytes
#   "sparse"   W_lo8 pruned 2:4 along K (the two largest of every four kept): the sparse matrix path, half the W_lo8 bytes
#   "tophalf"  the term only in the half of a matrix' 128-wide K-tiles with the largest ||W_lo[:, tile]||_F rms(A[.., tile]) (static per matrix)
#   "none"     no weight-side term (for scale)
# W_SIDE_ONLY: restrict the alternative form to these weight knobs (e.g. {"w_1"}); the others keep the engine's form.
W_SIDE_MODE = None
W_SIDE_ONLY = None
_cur_wknob = None


def _e2m1_mx(x, axis=-1, block=32):
    """MX-fp4: e2m1 (values 0, .5, 1, 1.5, 2, 3, 4, 6 x sign) with one shared power-of-two scale per `block` consecutive elements along `axis` (scale = 2^(floor(log2 max) - 2))."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    sh = x.shape
    pad = (-sh[-1]) % block
    if pad:
        x = np.concatenate([x, np.zeros(sh[:-1] + (pad,))], -1)
    xb = x.reshape(x.shape[:-1] + (-1, block))
    m = np.abs(xb).max(-1, keepdims=True)
    e = np.where(m > 0, np.floor(np.log2(np.where(m > 0, m, 1.0))) - 2.0, 0.0)
    y = xb / 2.0 ** e
    grid = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    a = np.minimum(np.abs(y), 6.0)
    idx = np.abs(a[..., None] - grid).argmin(-1)
    q = np.copysign(grid[idx], y) * 2.0 ** e
    q = q.reshape(x.shape)[..., :sh[-1]]
    return np.moveaxis(q, -1, axis)


def _wside_term(ah8, wl8, A):
    mode = W_SIDE_MODE if (W_SIDE_ONLY is None or _cur_wknob in W_SIDE_ONLY) else None
    if mode is None:
        return ah8 @ wl8.T
    if mode == "none":
        return 0.0
    if mode == "fp4":
        return _e2m1_mx(ah8) @ _e2m1_mx(wl8).T
    if mode == "sparse":
        w4 = wl8.reshape(wl8.shape[0], -1, 4)
        order = np.argsort(-np.abs(w4), -1)
        keep = np.zeros_like(w4, bool)
        np.put_along_axis(keep, order[..., :2], True, -1)
        return ah8 @ (w4 * keep).reshape(wl8.shape).T
    if mode == "tophalf":
        K = wl8.shape[1]
        nt = K // 128
        score = np.array([np.linalg.norm(wl8[:, t * 128:(t + 1) * 128]) * np.sqrt((A[..., t * 128:(t + 1) * 128] ** 2).mean()) for t in range(nt)])
        keep = np.zeros(K, bool)
        for t in np.argsort(-score)[: (nt + 1) // 2]:
            keep[t * 128:(t + 1) * 128] = True
        return ah8[..., keep] @ wl8[:, keep].T
    raise ValueError(mode)


def _mm_planes(afmt, ah, ah8, al8, W, sp_lo=None, rows=None, A=None, q_row_term=True):
    """The MV_F16X8 product of ``_mm`` from the A operand's PLANES as the engine holds them (tests/gemm_stage_kit.py hands over what a launch was given):
    ``ah`` the fp16 plane, ``ah8`` / ``al8`` the e4m3 planes de-scaled (hi8 2^-X8_ACT_SHIFT, lo8 2^-(11 + X8_ACT_SHIFT)), all float64 [B, S, K] (or [M, K]
    without a row term); ``W`` the float64 weight, rounded here (_w_planes).  ``sp_lo`` (float64 [B, R, K]): the fp16 value of 2^11 x the low part of the
    rows ``rows`` [B, R] of each sequence — the operand of their row term; None = no row term.  ``afmt`` as in _mm.  ``A``: the unrounded operand, read
    only by the model-side W_SIDE_MODE "tophalf"."""
    wh, wh8, wl8 = _w_planes(W)
    out = ah @ wh.T + _wside_term(ah8, wl8, ah + al8 if A is None else A)

    def cls_term(cols):
        if sp_lo is not None and ah.ndim == 3:
            bi = np.arange(ah.shape[0])
            for j in range(rows.shape[1]):
                r = rows[:, j]
                if j and (r == rows[:, 0]).all():
                    continue
                out[bi, r, cols] += (sp_lo[:, j] @ wh[cols].T) / 2048.0

    if afmt == "f16x8w":  # the weight-side term only (gemm_pp.h x8_terms = 1)
        cls_term(slice(None))
        return out
    if afmt != "f16x8":   # packed QKV weight [3 H][K]: the A-side term only in the Q / K / V block (gemm_pp.h x8_aside_mask)
        Hb = W.shape[0] // 3
        b = "qkv".index(afmt[-1])
        out[..., b * Hb:(b + 1) * Hb] += al8 @ wh8[b * Hb:(b + 1) * Hb].T
        if b != 0 or q_row_term:  # the engine forms the [CLS] row's term of the QKV projection only when the Q block lacks the A-side term (encoder_pass.h encode_dev:
            for o in range(3):  # K and V of the [CLS] token are one key among S); the launch skips it in the block that swept both terms
                if o != b:
                    cls_term(slice(o * Hb, (o + 1) * Hb))
        return out
    return out + al8 @ wh8.T


def _mm(afmt, wfmt, A, W, cls_lo=None, rows=None):
    """A @ W^T as the engine forms it.  Both operands "f16x8" (MV_F16X8): ONE fp16 sweep + two fp8 (e4m3) correction sweeps
    into the same fp32 accumulators,  A_hi W_hi + A_lo8 W_hi8 + A_hi8 W_lo8;  otherwise each operand is rounded on its own.
    ``cls_lo`` (the [CLS]-row form, engine.hip cls_aside; A is [B, S, K]): wherever the sweep carried the weight-side term only, row 0 of
    every sequence — its [CLS] token — gets the A-side term from a skinny fp16 GEMM  fp16(2^11 A_lo) fp16(W)^T 2^-11  with A_lo taken from
    the operand's lo fp16 plane ("lo16": the raw stream) or its lo8 plane ("lo8": context, GELU output).  ``rows`` (int [B, R], round 6): the rows of
    each sequence that get the term instead of row 0 alone (e.g. the [CLS] and the [SEP] token).  The arithmetic on the planes is _mm_planes."""
    if afmt in ("f16x8", "f16x8w", "f16x8q", "f16x8k", "f16x8v") and wfmt == "f16x8":
        ah, ah8, al8 = _x8_planes(A, X8_ACT_SHIFT)
        sp_lo, rr = None, rows
        if cls_lo and A.ndim == 3:
            rr = np.zeros((A.shape[0], 1), np.int64) if rows is None else rows
            bi = np.arange(A.shape[0])
            sp_lo = np.stack([_f16((_f16(A[bi, rr[:, j]] - ah[bi, rr[:, j]]) if cls_lo == "lo16" else al8[bi, rr[:, j]]) * 2048.0) for j in range(rr.shape[1])], 1)
        return _mm_planes(afmt, ah, ah8, al8, W, sp_lo, rr, A, q_row_term=rows is not None)
    return FORMATS[afmt](A) @ FORMATS[wfmt](W).T


def _split(x, rnd, n):
    out = np.zeros_like(x, dtype=np.float64)
    rem = x.astype(np.float64)
    for _ in range(n):
        part = rnd(rem)
        out += part
        rem = rem - part
    return out


FORMATS = {
    "exact": lambda x: x.astype(np.float64),
    "f16": _f16,
    "f16x2": lambda x: _split(x, _f16, 2),
    "bf16": _bf16,
    "bf16x2": lambda x: _split(x, _bf16, 2),
    "bf16x3": lambda x: _split(x, _bf16, 3),
    # one-sided use of the MV_F16X8 planes (the other operand in another format): hi + the de-scaled fp8 lo plane
    "f16x8": lambda x: (lambda p: p[0] + p[2])(_x8_planes(x, X8_ACT_SHIFT)),
    "f16x8w": _f16,  # an A operand whose own correction term is not swept: plain fp16 when paired with a non-x8 weight format
    "f16x8q": _f16, "f16x8k": _f16, "f16x8v": _f16,
}

# the knobs of the MV_F16X8 engine in its both-terms form (rounds 3-4; MEMVUL_CLS_ASIDE=0, and every sequence shorter than 128 tokens): every GEMM sweeps both
# first-order terms except the QKV projection, which sweeps the A-side term in its Q block only (the weight-side term everywhere)
X8_ENGINE = dict(w_qkv="f16x8", w_o="f16x8", w_1="f16x8", w_2="f16x8", a_qkv="f16x8q", a_ffn1="f16x8", ctx="f16x8", h="f16x8")

# ... and in the SHIPPED [CLS]-row form (round 5, the default; pass ``cls_fix=True`` to encode / logits with it): the weight-side term everywhere, the A-side
# term in the Q block of the QKV projection (all rows) and, through the skinny GEMMs, in the [CLS] row of every sequence for the other three GEMMs
X8_ENGINE_CLS = dict(w_qkv="f16x8", w_o="f16x8", w_1="f16x8", w_2="f16x8", a_qkv="f16x8q", a_ffn1="f16x8w", ctx="f16x8w", h="f16x8w")

# Round 6, the special rows: the formats of X8_ENGINE_CLS with THESE keyword arguments of encode / logits are the shipped default — the row terms go to the
# [CLS] AND the [SEP] row of every sequence (in the K / V blocks of the QKV projection too) and V of those two rows reaches attention as hi + lo
SHIPPED_KW = dict(cls_fix=True, special="cls+sep", special_v="f16x2", res_special="exact")
# ... and (round 6, second half) MV_F16X8 stores the residual stream of every OTHER row as hi fp16 + the lo8 plane of its fp8 planes (gemm.h GemmArgs::out16b): the knobs
# of the shipped default are X8_ENGINE_SHIPPED with SHIPPED_KW (res_special: the special rows keep hi + lo; with the "exact" stream of X8_ENGINE_CLS it changes nothing).
# scripts/r06_stream_model.py: this form models at the two-plane stream's error; the ordinary rows' stream as the hi plane ALONE (res="f16") at +14 % (GPU: +28 % on the
# median of 24 draws for +4 % issue reports/s: not taken); the hi plane alone in EVERY row at 3 - 6e-3
X8_ENGINE_SHIPPED = dict(X8_ENGINE_CLS, res="f16x8", a_qkv="f16x8w")
# (a_qkv: since the round's second half NO block of the QKV projection sweeps the A-side term for every row — MEMVUL_QKV_ASIDE's default is "none"; the special rows take it
# from their row term in all three blocks.  scripts/r06_qkv_model.py: q / none / qkv within 7 % of each other (mean rms) over 4 diffuse + 4 sink draws)

KNOBS = ("w_qkv", "w_o", "w_1", "w_2", "a_qkv", "a_ffn1", "qkv", "p", "ctx", "h", "res")
# (round 6) "q", "k", "v": the storage format of one of the three alone; each follows "qkv" unless given


def engine_formats(layers: int, fmt: str = "f16", **override) -> Dict[str, List[str]]:
    """The engine's shipped rounding points (every knob ``fmt`` in every layer) with per-knob overrides: a format
    name (all layers) or a list of per-layer names."""
    cfg = {k: [fmt] * layers for k in KNOBS}
    cfg["res"] = ["exact"] * layers  # (the two-plane fp16 stream is exact at this model's resolution: 2^-22)
    for k, v in override.items():
        cfg[k] = [v] * layers if isinstance(v, str) else list(v)
    for k in ("q", "k", "v"):
        cfg.setdefault(k, cfg["qkv"])
    return cfg


def _ln_stats(x, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return mu, 1.0 / np.sqrt(var + eps)


def encode(w, ids, mask, cfg: Optional[Dict[str, List[str]]], heads=12, eps=1e-12, fold_ln=True, cls_side=None, cls_raw_kv=False,
           cls_from_layer=0, cls_fix=False, special="cls", special_v=None, special_a_qkv=True, res_special=None, taps: Optional[dict] = None):
    """float64 BERT forward with the engine's rounding points (``cfg`` None = exact).  ``fold_ln``: the QKV / FFN-1
    weights are rounded AFTER the preceding LayerNorm is folded in (W'' = W gamma - rowmean, gemm_pp.h) and the A operand
    is the raw (pre-LayerNorm) stream, as on the engine's persistent-GEMM path.  ``cls_fix``: the [CLS]-row A-side term of the shipped form
    (see _mm) in every GEMM whose A format sweeps the weight-side term only; ``special`` = "cls" (row 0 of every sequence) or "cls+sep" (round 6:
    also its last token: the two tokens trained BERT heads use as attention sinks).  ``special_v`` (a format name, e.g. "f16x2"): V of the special rows is
    stored in that format instead of the ``v`` knob's (the attention kernel adds p[:, special] V_lo[special]: two rank-1 updates per head).  ``res_special`` (a format
    name): the special rows of the STORED residual stream keep that format while every other row follows the ``res`` knob (a model-side experiment of round 6: the stream
    of the ordinary rows as its hi plane alone).  ``taps`` (a dict): receives the NORMALISED stream of the main path after the embeddings (key 0) and after every
    layer (key n = after n layers: what the engine's debug tap 0 holds after ``debug_encode(ids, lens, n)``); nothing else changes."""
    W = lambda k: w[PFX + k].astype(np.float64)  # noqa: E731
    L = orc.n_layers(w)
    if cfg is None:
        cfg = engine_formats(L, "exact")
    def R(knob, l, x):
        y = FORMATS[cfg[knob][l]](x)
        if knob == "res" and res_special:
            rr = np.zeros((x.shape[0], 1), np.int64) if rows is None else rows
            for j in range(rr.shape[1]):
                y[np.arange(x.shape[0]), rr[:, j]] = FORMATS[res_special](x[np.arange(x.shape[0]), rr[:, j]])
        return y

    for k3 in ("q", "k", "v"):
        cfg.setdefault(k3, cfg["qkv"])
    B, S = ids.shape
    rows = None
    if special == "cls+sep":
        rows = np.stack([np.zeros(B, np.int64), mask.astype(np.int64).sum(1) - 1], 1)
    H = W("embeddings.word_embeddings.weight").shape[1]
    d = H // heads
    r = (W("embeddings.word_embeddings.weight")[ids] + W("embeddings.position_embeddings.weight")[np.arange(S)][None]
         + W("embeddings.token_type_embeddings.weight")[0][None, None])
    g, b = W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias")
    addmask = ((1.0 - mask.astype(np.float64)) * orc.MASK_ADD)[:, None, None, :]
    # [CLS] side path (cls_side = format name of ITS operands, e.g. "exact" / "f16x2"): the [CLS] row of every issue report
    # is re-computed in every layer at higher precision from the main path's stored K / V of all tokens; the pooler reads
    # the side path's row.  The main path does not depend on it.  ``cls_from_layer``: the side path starts at that layer from the
    # main path's [CLS] row (L - 1 = only the last layer's [CLS] work at the higher precision: the engine's pruned tail).
    rc = r[:, 0].copy()
    gc, bc = g, b
    RS = FORMATS[cls_side] if cls_side else None

    def tap(n, r, g, b):
        if taps is not None:
            mu, rstd = _ln_stats(r, eps)
            taps[n] = (r - mu) * rstd * g + b

    tap(0, r, g, b)

    def consumer(r_raw, g, b, Wm, bias, wknob, aknob, l):
        """rstd * (W'' · round(r)) + b'  ==  W · LN(r) + bias  up to the roundings"""
        global _cur_wknob
        _cur_wknob = wknob
        mu, rstd = _ln_stats(r_raw, eps)
        if fold_ln:
            Wg = Wm * g[None, :]
            bf = bias + Wm @ b
            return rstd * _mm(cfg[aknob][l], cfg[wknob][l], r_raw, Wg - Wg.mean(-1, keepdims=True), "lo16" if cls_fix else None, rows) + bf
        x = (r_raw - mu) * rstd * g + b
        return _mm(cfg[aknob][l], cfg[wknob][l], x, Wm, "lo16" if cls_fix else None, rows) + bias

    for l in range(L):
        p = f"encoder.layer.{l}."
        Wqkv = np.concatenate([W(p + "attention.self.query.weight") * 0.125, W(p + "attention.self.key.weight"),
                               W(p + "attention.self.value.weight")], 0)
        bqkv = np.concatenate([W(p + "attention.self.query.bias") * 0.125, W(p + "attention.self.key.bias"),
                               W(p + "attention.self.value.bias")], 0)
        r_in = r
        if cls_side and l == cls_from_layer and l > 0:
            rc, gc, bc = r[:, 0].copy(), g, b
        qkv = consumer(r, g, b, Wqkv, bqkv, "w_qkv", "a_qkv", l)
        vst = R("v", l, qkv[..., 2 * H:])
        if special_v:
            rr = np.zeros((B, 1), np.int64) if rows is None else rows
            for j in range(rr.shape[1]):
                vst[np.arange(B), rr[:, j]] = FORMATS[special_v](qkv[np.arange(B), rr[:, j], 2 * H:])
        qkv = np.concatenate([R("q", l, qkv[..., :H]), R("k", l, qkv[..., H:2 * H]), vst], -1)
        sp = lambda t: t.reshape(B, S, heads, d).transpose(0, 2, 1, 3)  # noqa: E731
        qh, kh, vh = sp(qkv[..., :H]), sp(qkv[..., H:2 * H]), sp(qkv[..., 2 * H:])
        sc = qh @ kh.transpose(0, 1, 3, 2) + addmask  # 1/sqrt(d) folded into W_q (exact power of two)
        m = sc.max(-1, keepdims=True)
        e = np.exp(sc - m)
        den = e.sum(-1, keepdims=True)
        ctx = ((R("p", l, e) @ vh) / den).transpose(0, 2, 1, 3).reshape(B, S, H)  # the engine normalises O after P·V
        mu, rstd = _ln_stats(r, eps)
        x = (R("res", l, r) - mu) * rstd * g + b  # the residual GEMM reads the STORED stream; its statistics come from the accumulators
        global _cur_wknob
        _cur_wknob = "w_o"
        r1 = _mm(cfg["ctx"][l], cfg["w_o"][l], ctx, W(p + "attention.output.dense.weight"), "lo8" if cls_fix else None, rows) + W(p + "attention.output.dense.bias") + x
        g1, b1 = W(p + "attention.output.LayerNorm.weight"), W(p + "attention.output.LayerNorm.bias")
        hpre = consumer(r1, g1, b1, W(p + "intermediate.dense.weight"), W(p + "intermediate.dense.bias"), "w_1", "a_ffn1", l)
        h = orc._gelu(hpre)
        mu, rstd = _ln_stats(r1, eps)
        x1 = (R("res", l, r1) - mu) * rstd * g1 + b1
        _cur_wknob = "w_2"
        r = _mm(cfg["h"][l], cfg["w_2"][l], h, W(p + "output.dense.weight"), "lo8" if cls_fix else None, rows) + W(p + "output.dense.bias") + x1
        if cls_side and l >= cls_from_layer:
            mu, rstd = _ln_stats(rc, eps)
            xc = (rc - mu) * rstd * gc + bc
            qc = (RS(xc) @ RS(Wqkv[:H]).T + bqkv[:H]).reshape(B, heads, 1, d)
            khc, vhc = kh, vh
            if cls_raw_kv:  # the [CLS] row attends to the main path's RAW stream: K / V re-derived at the side path's precision
                mu, rstd = _ln_stats(r_in, eps)
                xm = RS((r_in - mu) * rstd * g + b)
                khc = sp(xm @ RS(Wqkv[H:2 * H]).T + bqkv[H:2 * H])
                vhc = sp(xm @ RS(Wqkv[2 * H:]).T + bqkv[2 * H:])
            scc = qc @ khc.transpose(0, 1, 3, 2) + addmask
            ec = np.exp(scc - scc.max(-1, keepdims=True))
            cc = ((ec @ vhc) / ec.sum(-1, keepdims=True)).reshape(B, H)
            r1c = RS(cc) @ RS(W(p + "attention.output.dense.weight")).T + W(p + "attention.output.dense.bias") + xc
            mu, rstd = _ln_stats(r1c, eps)
            x1c = (r1c - mu) * rstd * g1 + b1
            hc = orc._gelu(RS(x1c) @ RS(W(p + "intermediate.dense.weight")).T + W(p + "intermediate.dense.bias"))
            rc = RS(hc) @ RS(W(p + "output.dense.weight")).T + W(p + "output.dense.bias") + x1c
        g, b = W(p + "output.LayerNorm.weight"), W(p + "output.LayerNorm.bias")
        gc, bc = g, b
        tap(l + 1, r, g, b)
    if cls_side:
        r = r.copy()
        r[:, 0] = rc
    mu, rstd = _ln_stats(r, eps)
    return (r - mu) * rstd * g + b


def instance_forward(w, ids, mask, cfg=None, **kw):
    h = encode(w, ids, mask, cfg, **kw)
    pooled = np.tanh(h[:, 0] @ w[orc_key("pool_w")].astype(np.float64).T + w[orc_key("pool_b")].astype(np.float64))
    return np.maximum(pooled @ w[orc_key("head_w")].astype(np.float64).T + w[orc_key("head_b")].astype(np.float64), 0)


def orc_key(name):
    return {"pool_w": "_bert_pooler.pooler.dense.weight", "pool_b": "_bert_pooler.pooler.dense.bias",
            "head_w": "_projector_single._linear_layers.0.weight", "head_b": "_projector_single._linear_layers.0.bias"}[name]


def logits(w, ids, mask, aids, amask, cfg=None, **kw):
    u = instance_forward(w, ids, mask, cfg, **kw)
    v = instance_forward(w, aids, amask, cfg, **kw)
    return orc.match(u, v, w["_projector.weight"].astype(np.float64))[0], u, v
