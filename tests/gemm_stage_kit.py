"""Shared pieces of the GEMM stage tests (tests/test_gemm_stage_cpu.py, tests/test_gemm_stage_gpu.py): each of the four persistent GEMM launches of a layer —
QKV projection, output projection, FFN-1, FFN-2 (gemm_pp.h) — against a float64 model formed from THAT LAUNCH'S OWN operands: the planes the launch was
handed (fp16 hi plane, the fp8 planes, the special rows' compact low parts, the row statistics), through oracle/precision_model.py _mm_planes, compared with the
planes the launch wrote.  Plain module: no fixtures, no GPU.

A launch is described by a record (a dict of float64 arrays in TOKEN order, [B, Sp, ...]; the fp8 planes decoded and de-scaled; the compact special-row
buffers as [B, 2, N] holding 2^11 x the low part, row 0 = the [CLS] token, row 1 = the last token — token 1 for a sequence of fewer than 3):
  inputs   a_hi, a_hi8, a_lo8, a_sp (the row term's operand), stats [B, Sp, 3, 2]; the residual GEMMs also s_hi, s_lo8, s_sp, s_lo (MV_F16) of the stream
  outputs  QKV: q, k, v (+ q_lo, k_lo, v_lo, vlo_sp);  residual: hi, hi8, lo8, sp, lo (MV_F16), stats_out;  FFN-1: hi, hi8, lo8, sp
read_state() / layer_records() fill them from an engine stopped between the launches (MEMVUL_DEBUG_STOP), emulate_*() from a numpy emulation of the kernel's arithmetic.

Which rows take which form is stated HERE from the documented rule (pass_form), never read from the engine.

The bounds are per element: the storage rounding of the output plus the fp32-accumulation allowance (allowance())
  ACC x rms(pre-activation of the launch)  [residual GEMMs: + 3 sqrt(R / 12) 2^-23 |x|, R = the fp32 roundings of the accumulator],  ACC = 3e-5
— the first term the project's allowance for "the kernel forms exactly the modelled product" (tests/test_gpu_kernels.py test_persistent_gemm_fp16_and_fp8_correction_sweep);
tests/test_gemm_stage_cpu.py holds a float32 emulation at or below 0.9 of every bound at K = 768 and K = 3072 and with the in-situ rstd x acc + b' step, so the
constant is not raised.  Storage roundings: half an fp16 ulp at the stored value where one plane is stored; |x| 2^-15 + 2^-22 where hi + the lo8 plane is;
|x| 2^-22 + 2^-25 where hi + lo fp16 is (lo = fp16(x - hi), |x - hi| <= 2^-11 |x|, half an ulp of that or half a subnormal step)."""
import numpy as np

from oracle import memvul_oracle as orc
from oracle import precision_model as pm

H, INTER, HEADS, HD = 768, 3072, 12, 64
ACC = 3e-5           # fp32-accumulation allowance, x rms(pre-activation): see the module docstring for its source
CLS_MIN_LEN = 128    # MEMVUL_CLS_ASIDE_MIN_LEN's default
LN_EPS = 1e-12
SH = 2.0 ** pm.X8_ACT_SHIFT
LAUNCHES = ("qkv", "out_proj", "ffn1", "ffn2")
CLASSES = ("special", "both", "wside")


def padded_len(S):
    return (S + 63) // 64 * 64 if S <= 256 else (S + 127) // 128 * 128


def e4m3_decode(b):
    """OCP e4m3fn bytes -> float64 (0x7f / 0xff = NaN)."""
    b = np.asarray(b, np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b >> 7, -v, v)


def special_rows(lens):
    """int [B, 2]: the tokens in the engine's rows 0 and 1 of every sequence (embed_ln_kernel: the last token is computed in row 1 when len >= 3)."""
    lens = np.asarray(lens, np.int64)
    return np.stack([np.zeros_like(lens), np.where(lens >= 3, lens - 1, 1)], 1)


# ---- the documented rule: which rows take which form --------------------------------------------------------------------------------------------------------------

def pass_form(engine, Sp, lens, cls_aside=True, qkv_aside=""):
    """engine "precise" | "safe" | "f16".  Returns dict(x8, safe, two_plane, cls_as, both [B] bool, tile_both int [Mpad / 256] or None, qkv_mask):
    * the [CLS]-row form (cls_as) is in force for a pass of MV_F16X8's default form at padded length 256 / 512 — there per SEQUENCE: one shorter than
      MEMVUL_CLS_ASIDE_MIN_LEN keeps both terms (its 256-row tiles are flagged in tile_both) — and at 192 / 384 for the WHOLE pass when its shortest sequence
      has that many tokens; passes of 64 / 128, the safe form and MEMVUL_CLS_ASIDE=0 sweep both terms in every row;
    * both[b]: the output projection, FFN-1 and FFN-2 sweep the A-side term for the rows of sequence b (else: the special rows take it from their row term);
    * qkv_mask: the blocks of the QKV projection that sweep the A-side term for every row (bit 0 / 1 / 2 = Q / K / V): MEMVUL_QKV_ASIDE (default none), 7 in
      the safe form; the special rows take the row term in the other blocks;
    * two_plane: Q, K, V^T leave as hi + lo (the safe form; the default form up to 128)."""
    lens = np.asarray(lens)
    B = len(lens)
    x8 = engine in ("precise", "safe")
    safe = engine == "safe"
    f = dict(x8=x8, safe=safe, two_plane=safe or (x8 and Sp <= 128), cls_as=False, both=np.ones(B, bool), tile_both=None, qkv_mask=0)
    if not x8:
        return f
    f["qkv_mask"] = 7 if safe else sum({"q": 1, "k": 2, "v": 4}[c] for c in qkv_aside)
    if safe or not cls_aside:
        return f
    if Sp in (256, 512):
        f["cls_as"] = True
        f["both"] = lens < CLS_MIN_LEN
        ntile = (B * Sp + 255) // 256
        f["tile_both"] = np.array([int(any(lens[b] < CLS_MIN_LEN for b in range(t * 256 // Sp, min((t * 256 + 255) // Sp, B - 1) + 1))) for t in range(ntile)], np.int32)
    elif Sp in (192, 384) and lens.min() >= CLS_MIN_LEN:
        f["cls_as"] = True
        f["both"] = np.zeros(B, bool)
    return f


def row_classes(lens, Sp, form):
    """bool [B, Sp] masks of the real rows: special (rows 0 and the last token), both (A-side term swept), wside (weight-side term only); and pad (rows >= len)."""
    lens = np.asarray(lens)
    B = len(lens)
    real = np.arange(Sp)[None, :] < lens[:, None]
    sp = np.zeros((B, Sp), bool)
    rr = special_rows(lens)
    sp[np.arange(B), rr[:, 0]] = True
    sp[np.arange(B), rr[:, 1]] = True
    sp &= real
    both = np.broadcast_to(form["both"][:, None], (B, Sp))
    return dict(special=sp, both=real & ~sp & both, wside=real & ~sp & ~both, pad=~real)


# ---- the weights of a layer, as the engine prepares them ------------------------------------------------------------------------------------------------------------

def layer_weights(w, l):
    """float64 matrices of layer l (0-based) as weights.h prepares them: W'' = W gamma - rowmean, b' = b + W beta folded in double and kept as float32 (the planes
    are then pm._w_planes of that), W_q / b_q scaled by 1 / 8; pend_g / pend_b: the LayerNorm pending on the stream the layer reads."""
    W = lambda k: w[pm.PFX + k].astype(np.float64)  # noqa: E731
    p = f"encoder.layer.{l}."
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731

    def fold(Wm, bias, g, b):
        Wg = Wm * g[None, :]
        return f32(Wg - Wg.mean(-1, keepdims=True)), f32(bias + Wm @ b)

    if l == 0:
        g, b = W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias")
    else:
        g, b = W(f"encoder.layer.{l - 1}.output.LayerNorm.weight"), W(f"encoder.layer.{l - 1}.output.LayerNorm.bias")
    Wqkv = np.concatenate([W(p + "attention.self.query.weight") * 0.125, W(p + "attention.self.key.weight"), W(p + "attention.self.value.weight")], 0)
    bqkv = np.concatenate([W(p + "attention.self.query.bias") * 0.125, W(p + "attention.self.key.bias"), W(p + "attention.self.value.bias")], 0)
    g1, b1 = W(p + "attention.output.LayerNorm.weight"), W(p + "attention.output.LayerNorm.bias")
    out = dict(pend_g=g, pend_b=b, ln1g=g1, ln1b=b1, wo=W(p + "attention.output.dense.weight"), bo=W(p + "attention.output.dense.bias"),
               w2=W(p + "output.dense.weight"), b2=W(p + "output.dense.bias"))
    out["wqkv"], out["bqkv"] = fold(Wqkv, bqkv, g, b)
    out["w1"], out["b1"] = fold(W(p + "intermediate.dense.weight"), W(p + "intermediate.dense.bias"), g1, b1)
    return out


# ---- float64 models of the launches ---------------------------------------------------------------------------------------------------------------------------------

def ln_stats64(stats):
    """(mean, rstd) [B, Sp, 1] in float64 by the rule of common.h ln_from_partials, from the engine's own three (sum, sum of squares) pairs."""
    s = np.asarray(stats, np.float64)
    s1, s2 = s[..., 0].sum(-1), s[..., 1].sum(-1)
    mean = s1 / H
    var = np.maximum(s2 / H - mean * mean, 0.0)
    return mean[..., None], (1.0 / np.sqrt(var + LN_EPS))[..., None]


def product64(rec, Wm, form, lens, qkv=False, col0=0):
    """A (x) W^T of the launch in float64 from its planes: [B, Sp, N].  col0 = 768: the K / V-only QKV launch (every block weight-side only + the row term)."""
    a_hi = rec["a_hi"]
    if not form["x8"]:
        return a_hi @ pm._f16(Wm).T
    rows = special_rows(lens)
    if qkv:
        m = form["qkv_mask"]
        assert m in (0, 1, 7), "the forms the tests run: MEMVUL_QKV_ASIDE none / q, the safe form"
        afmt = {0: "f16x8w", 1: "f16x8q", 7: "f16x8"}[m]
        assert col0 == 0 or m == 0
        return pm._mm_planes(afmt, a_hi, rec["a_hi8"], rec["a_lo8"], Wm, None if m == 7 else rec["a_sp"], rows)
    out = np.empty(a_hi.shape[:2] + (Wm.shape[0],))
    for both in (True, False):
        idx = np.nonzero(form["both"] == both)[0]
        if len(idx):
            out[idx] = pm._mm_planes("f16x8" if both else "f16x8w", a_hi[idx], rec["a_hi8"][idx], np.nan_to_num(rec["a_lo8"][idx]) if both else np.zeros_like(a_hi[idx]),
                                     Wm, None if both else rec["a_sp"][idx], rows[idx], A=a_hi[idx])  # (A: read by the model-side W_SIDE_MODE "tophalf" alone)
    return out


def stream64(rec, lens, form, pfx="s_"):
    """The stored raw stream decoded: hi + lo8 2^-(11 + shift) (already de-scaled), the special rows hi + sp 2^-11; MV_F16: hi + lo."""
    hi = rec[pfx + "hi"] if pfx else rec["hi"]
    if not form["x8"]:
        return hi + rec[pfx + "lo"]
    x = hi + rec[pfx + "lo8"]
    rows = special_rows(lens)
    bi = np.arange(len(lens))
    for j in (1, 0):
        x[bi, rows[:, j]] = hi[bi, rows[:, j]] + rec[pfx + "sp"][:, j] / 2048.0
    return x


def model_qkv(rec, lw, form, lens, col0=0):
    _, rstd = ln_stats64(rec["stats"])
    return rstd * product64(rec, lw["wqkv"][col0:], form, lens, qkv=True, col0=col0) + lw["bqkv"][col0:]


def model_residual(rec, Wm, bias, g, b, form, lens):
    mean, rstd = ln_stats64(rec["stats"])
    return product64(rec, Wm, form, lens) + bias + ((stream64(rec, lens, form) - mean) * rstd * g + b)


def model_ffn1(rec, lw, form, lens):
    _, rstd = ln_stats64(rec["stats"])
    pre = rstd * product64(rec, lw["w1"], form, lens) + lw["b1"]
    return pre, orc._gelu(pre)


# ---- the bounds -----------------------------------------------------------------------------------------------------------------------------------------------------

def rms_real(x, lens):
    real = np.arange(x.shape[1])[None, :] < np.asarray(lens)[:, None]
    return float(np.sqrt((x[real] ** 2).mean()))


ROUNDINGS_PER_MFMA = 8  # fp32 roundings of an accumulator per MFMA instruction (a 16x16x32 fp16 instruction runs as 8 passes of 4 K-elements): see allowance()


def allowance(rms, K, residual=False):
    """The fp32-accumulation allowance of an element whose modelled value is m:  ACC x rms(pre-activation)  [+ 3 sqrt(R / 12) 2^-23 |m|  for a residual GEMM].
    The first term is the project's (module docstring) and is all a RAW launch (QKV projection, FFN-1) gets: its accumulators start from zero.
    A residual GEMM (PP_RESLN3) parks bias + LayerNorm(residual) — the element's full magnitude — in the accumulator BEFORE the sweeps, so every later rounding
    of the accumulator is a rounding of |m|, whatever the products add: half an fp32 ulp <= 2^-24 |m| each, uniform, R = ROUNDINGS_PER_MFMA x (K / 32 + K / 64)
    of them (fp16 sweep 16x16x32, fp8 sweep 16x16x128 with both terms) — a random walk with sigma = sqrt(R / 12) 2^-23 |m|, taken at 3 sigma.  The rms cannot
    stand for it when an element is many times the rms (LayerNorm outlier dimensions: 27 rms on the outliers2 model), and only a storage finer than 2^-15 of
    the element shows it: the special rows' hi + lo.  R was settled by running the emulation on the ENGINE's own planes (outliers2, FFN-2 and the output
    projection of both layers at 64 and 256 keys) with 1, 2, 4, 8 roundings per instruction: the engine's relative rms error on the special rows' elements
    above 8 (K = 3072: 6.2, 7.9, 5.4, 4.2e-7; K = 768: 2.6, 3.5, 1.8, 2.0e-7), unbiased, lies between 4 (4.6, 5.0, 3.4, 5.1e-7) and 8 (7.8, 7.8, 9.4, 6.5e-7)
    and at twice what one rounding per instruction gives (3.2, 3.4, 3.0, 1.9e-7) — profiles/gemm_stage_parity.md; the emulation (emulate_*: MFMA_SPLIT) rounds
    8 times per instruction since, and tests/test_gemm_stage_cpu.py holds THAT emulation at 0.9 of this allowance on an outlier stream."""
    if not residual:
        return lambda m: ACC * rms + 0.0 * np.abs(m)
    R = ROUNDINGS_PER_MFMA * (K // 32 + K // 64)
    return lambda m: ACC * rms + 3.0 * np.sqrt(R / 12.0) * 2.0 ** -23 * np.abs(m)


def half_ulp16(stored):
    """Half an fp16 ulp AT the stored value (float64 in, exactly representable): what the one-plane store itself may have moved the element by."""
    return np.spacing(np.abs(stored).astype(np.float16)).astype(np.float64) / 2.0


def store_hi_lo8(m):
    """hi + the lo8 plane: the 4 significant bits of e4m3((x - hi) 2^(11 + shift)) leave 2^-4 of |x - hi| <= 2^-11 |x|, or half its subnormal step."""
    return 2.0 ** -15 * np.abs(m) + 2.0 ** -22


def store_hi_lo(m):
    """hi + lo fp16: lo = fp16(x - hi), |x - hi| <= 2^-11 |x|: half an ulp of that, or half a subnormal step."""
    return 2.0 ** -22 * np.abs(m) + 2.0 ** -25


def bound_hi8(hi):
    """hi8 = e4m3 of the value whose fp16 is hi: half an e4m3 ulp (3 mantissa bits: 2^-4 |x|), its subnormal step 2^-9 / 2^shift; + the fp16 half ulp between
    the accumulator the kernel converts and the stored hi."""
    return np.abs(hi) * (2.0 ** -4 + 2.0 ** -11) + 2.0 ** -10 / SH


class Report:
    """Per (launch, quantity, row class): the bound of an element is  storage rounding + allow  (allow = allowance(...)(modelled value)).  A
    storage rounding fills its own share of such a bound by construction (an element that sits just below half an ulp), so what is reported and asserted is the
    share of the ALLOWANCE the element needs:  ratio = max(0, |engine - model| - storage) / allow  — ratio <= 1 is exactly |engine - model| <= bound, and the
    emulation's 0.9 is asked of the part the constant ACC stands for.  allow None (vstats, hi8: bounds without an accumulation part): ratio = err / storage."""

    def __init__(self):
        self.rows = []

    def add(self, launch, what, err, storage, allow, classes, only=CLASSES, m=None):
        self._m = m  # the modelled values the allowance is a function of (allow not None)
        ratio = err / storage if allow is None else np.maximum(err - storage, 0.0) / allow(self._m)
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        for c in only:
            m = classes[c]
            if err.ndim == 3 and m.ndim == 2:
                m = np.broadcast_to(m[..., None], err.shape)
            if m.any():
                r = ratio[m]
                self.rows.append(dict(launch=launch, what=what, cls=c, max_ratio=float(r.max()), rms_ratio=float(np.sqrt((r ** 2).mean())),
                                      max_err=float(err[m].max()), rounding_only=allow is None))

    def worst(self, launch=None, cls=None, what=None, rounding_only=None):
        v = [r["max_ratio"] for r in self.rows if (launch is None or r["launch"] == launch) and (cls is None or r["cls"] == cls) and (what is None or r["what"] == what)
             and (rounding_only is None or r["rounding_only"] == rounding_only)]
        return max(v) if v else 0.0

    def by_launch_class(self, rounding_only=False):
        """{(launch, row class): (max, rms) of the ratios} over the quantities with an allowance (or over the rounding-only ones)."""
        out = {}
        for r in self.rows:
            if r["rounding_only"] != rounding_only:
                continue
            k = (r["launch"], r["cls"])
            out[k] = (max(out.get(k, (0, 0))[0], r["max_ratio"]), max(out.get(k, (0, 0))[1], r["rms_ratio"]))
        return out


def _special_compact(x, lens):
    """[B, Sp, N] -> the special rows [B, 2, N]."""
    rows = special_rows(lens)
    bi = np.arange(len(lens))
    return np.stack([x[bi, rows[:, 0]], x[bi, rows[:, 1]]], 1)


def _special_mask(lens):
    """bool [B, 2]: the compact row is a real token (row 1 of a one-token sequence is not)."""
    lens = np.asarray(lens)
    return np.stack([lens >= 1, lens >= 2], 1)


def check_qkv(rep, rec, lw, form, lens, col0=0):
    """Q, K, V (taps 2 - 4, + 7 - 9 where the pass wrote them) against rstd (A (x) W'') + b'; vlo_sp against V of the special rows.  col0 = 768: K and V of the
    K / V-only launch."""
    m = model_qkv(rec, lw, form, lens, col0)
    names = "qkv"[col0 // H:]
    Sp = m.shape[1]
    allow = allowance(rms_real(m, lens), H)
    cl = row_classes(lens, Sp, form)
    for i, nm in enumerate(names):
        mb = m[..., i * H:(i + 1) * H]
        # the classes of THIS block: it swept the A-side term for every row when its bit of qkv_mask is set
        c = dict(cl)
        if form["x8"]:
            swept = bool((form["qkv_mask"] >> (i + col0 // H)) & 1)
            real = ~cl["pad"] & ~cl["special"]
            c["both"], c["wside"] = (real, np.zeros_like(real)) if swept else (np.zeros_like(real), real)
        if form["two_plane"]:
            rep.add("qkv", nm + "_hi_lo", np.abs(rec[nm] + rec[nm + "_lo"] - mb), store_hi_lo(mb), allow, c, m=mb)
            rep.add("qkv", nm + "_lo", np.abs(rec[nm + "_lo"]), half_ulp16(rec[nm]) * (1.0 + 2.0 ** -10), None, c)  # lo = fp16(x - hi): at most half an ulp of hi, rounded
        else:
            rep.add("qkv", nm, np.abs(rec[nm] - mb), half_ulp16(rec[nm]), allow, c, m=mb)
    if rec.get("vlo_sp") is not None:
        mv = _special_compact(m[..., -H:], lens)
        got = _special_compact(rec["v"], lens) + rec["vlo_sp"] / 2048.0
        rep.add("qkv", "vlo_sp", np.abs(got - mv), store_hi_lo(mv), allow, dict(special=_special_mask(lens)), only=("special",), m=mv)
    return m


def _check_planes(rep, launch, rec, m, allow, form, lens, cl, lo8_rows):
    """The planes of a producer (residual GEMM, FFN-1) against the modelled value m: hi alone, hi + lo8 on the rows lo8_rows [B, Sp] whose lo8 plane the launch
    writes, hi + the compact low parts on the special rows (where the launch wrote them), hi8 against hi."""
    rep.add(launch, "hi", np.abs(rec["hi"] - m), half_ulp16(rec["hi"]), allow, cl, m=m)
    if not form["x8"]:
        return
    c8 = {k: v & lo8_rows for k, v in cl.items()}
    rep.add(launch, "hi_lo8", np.abs(rec["hi"] + rec["lo8"] - m), store_hi_lo8(m), allow, c8, only=("both", "wside"), m=m)
    rep.add(launch, "hi8", np.abs(rec["hi8"] - rec["hi"]), bound_hi8(rec["hi"]), None, cl)
    if rec.get("sp") is not None:
        ms = _special_compact(m, lens)
        got = _special_compact(rec["hi"], lens) + rec["sp"] / 2048.0
        rep.add(launch, "sp_lo", np.abs(got - ms), store_hi_lo(ms), allow, dict(special=_special_mask(lens)), only=("special",), m=ms)


def check_residual(rep, launch, rec, Wm, bias, g, b, form, lens):
    """Output projection / FFN-2: the stored stream after the launch against A (x) W + b + LN_pending(stream_in); the new rows' vstats against the sums of the
    STORED row (both planes: the accumulators to the storage rounding), per row and 256-column tile."""
    m = model_residual(rec, Wm, bias, g, b, form, lens)
    Sp = m.shape[1]
    allow = allowance(rms_real(m, lens), Wm.shape[1], residual=True)
    cl = row_classes(lens, Sp, form)
    real = ~cl["pad"]
    _check_planes(rep, launch, rec, m, allow, form, lens, cl, real)  # (the stream's lo8 plane is its low part in every form: out8_hi_only stays 0)
    if not form["x8"]:
        rep.add(launch, "hi_lo", np.abs(rec["hi"] + rec["lo"] - m), store_hi_lo(m), allow, cl, m=m)
    # vstats: (sum, sum of squares) of the fp32 accumulators.  Reference: the stored row decoded, which differs from the accumulator by the storage residual
    # res_j (uniform within +- its bound, independent between elements): 6 sigma of the sum, + the fp32 summation itself (22 sequential additions per lane and
    # tree level at most: 2^-20 of the sum of magnitudes)
    stored = stream64(rec, lens, form, pfx="")
    res = (2.0 ** -15 * np.abs(stored) + 2.0 ** -22) if form["x8"] else (2.0 ** -22 * np.abs(stored) + 2.0 ** -25)
    if form["x8"]:
        rows = special_rows(lens)
        for j in (0, 1):
            bi = np.arange(len(lens))
            res[bi, rows[:, j]] = 2.0 ** -22 * np.abs(stored[bi, rows[:, j]]) + 2.0 ** -25
    t = lambda x: x.reshape(x.shape[0], Sp, 3, 256)  # noqa: E731
    s1, s2 = t(stored).sum(-1), (t(stored) ** 2).sum(-1)
    b1 = 6.0 * np.sqrt((t(res) ** 2).sum(-1) / 3.0) + 2.0 ** -20 * np.abs(t(stored)).sum(-1)
    b2 = 6.0 * np.sqrt(((2.0 * t(stored) * t(res)) ** 2).sum(-1) / 3.0) + 2.0 ** -20 * s2
    so = rec["stats_out"]
    rep.add(launch, "vstats_sum", np.abs(so[..., 0] - s1), b1, None, cl)
    rep.add(launch, "vstats_sumsq", np.abs(so[..., 1] - s2), b2, None, cl)
    return m


def check_ffn1(rep, rec, lw, form, lens):
    """tap 6 against gelu(rstd (A (x) W'') + b'); h8: hi8 in every row, lo8 only where the launch writes it — every row without the [CLS]-row form, the rows of a
    tile flagged in tile_both with it (out8_hi_only); cls_lo against the GELU output's low parts of the special rows in that form."""
    pre, m = model_ffn1(rec, lw, form, lens)
    Sp = m.shape[1]
    allow = allowance(rms_real(pre, lens), H)
    cl = row_classes(lens, Sp, form)
    lo8_rows = np.broadcast_to(form["both"][:, None], (len(lens), Sp)) if form["cls_as"] else ~cl["pad"]
    _check_planes(rep, "ffn1", rec, m, allow, form, lens, cl, lo8_rows)
    return pre, m


# ---- reading a stopped engine ---------------------------------------------------------------------------------------------------------------------------------------

def _planes8(raw, K):
    """bytes [B, Sp, 2 K] = [lo8 | hi8] -> (hi8, lo8) de-scaled float64."""
    return e4m3_decode(raw[..., K:]) / SH, e4m3_decode(raw[..., :K]) / (2048.0 * SH)


def _heads_to_rows(x, vt=False):
    """[B, 12, Sp, 64] (or V^T [B, 12, 64, Sp]) -> [B, Sp, 768]."""
    if vt:
        x = x.transpose(0, 1, 3, 2)
    B, _, Sp, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, Sp, H)


def read_state(eng, form, want, seqs=None, tokens=None):
    """The buffers `want` (names) of a stopped engine as float64 in token order.  seqs (an index array): only these sequences of the batch; tokens (int [B, 2]):
    only these two tokens of every sequence (the per-token planes come back as [B, 2, ...]: a pass of two-token sequences).  Both subsets are taken from the
    raw planes, before anything is decoded."""
    B = len(eng._dbg[2])

    def sub(x, ax=1):
        if seqs is not None:
            x = x[np.asarray(seqs)]
        if tokens is not None and ax is not None:
            t = np.asarray(tokens) if seqs is None else np.asarray(tokens)[np.asarray(seqs)]
            x = np.take_along_axis(x, t.reshape([t.shape[0]] + [1] * (ax - 1) + [2] + [1] * (x.ndim - ax - 1)), axis=ax)
        return x

    f64 = lambda i, ax=1: sub(eng.debug_read(i), ax).astype(np.float64)  # noqa: E731
    compact = lambda i, N: sub(eng.debug_read(i)[:2 * B * N].reshape(B, 2, N), None).astype(np.float64)  # noqa: E731
    out = {}
    for nm in want:
        if nm == "x16":
            out[nm] = f64(1)
        elif nm == "x8":
            out["x_hi8"], out["x_lo8"] = _planes8(sub(eng.debug_read(11)), H)
        elif nm == "st_lo":
            out[nm] = compact(12, H)
        elif nm == "xlo":
            out[nm] = f64(19)
        elif nm == "lnstats":
            out[nm] = f64(13)
        elif nm == "lnpart":
            out[nm] = f64(14)
        elif nm == "ctx":
            out[nm] = f64(5)
        elif nm == "ctx8":
            out["ctx_hi8"], out["ctx_lo8"] = _planes8(sub(eng.debug_read(15)), H)
        elif nm in ("cls_lo768", "cls_lo3072"):
            out[nm] = compact(16, int(nm[6:]))
        elif nm == "h16":
            out[nm] = f64(6)
        elif nm == "h8":
            out["h_hi8"], out["h_lo8"] = _planes8(sub(eng.debug_read(17)), INTER)
        elif nm == "qkv":
            out["q"], out["k"], out["v"] = _heads_to_rows(f64(2, 2)), _heads_to_rows(f64(3, 2)), _heads_to_rows(f64(4, 3), vt=True)
            if form["two_plane"]:
                out["q_lo"], out["k_lo"], out["v_lo"] = _heads_to_rows(f64(7, 2)), _heads_to_rows(f64(8, 2)), _heads_to_rows(f64(9, 3), vt=True)
        elif nm == "vlo_sp":
            v = f64(18, None)
            out[nm] = v.transpose(0, 3, 1, 2).reshape(v.shape[0], 2, H)  # [B, 12, 64, 2] -> [B, 2, 768]
        elif nm == "tile_both":
            out[nm] = eng.debug_read(21)
        else:
            raise KeyError(nm)
    return out


def stream_rec(st, form, pfx):
    """The stream planes of a state as record fields with prefix pfx ("s_" = the residual a launch reads, "" = what it wrote)."""
    r = {pfx + "hi": st["x16"]}
    if form["x8"]:
        r.update({pfx + "hi8": st["x_hi8"], pfx + "lo8": st["x_lo8"], pfx + "sp": st["st_lo"]})
    else:
        r[pfx + "lo"] = st["xlo"]
    return r


STREAM = ("x16", "x8", "st_lo")


def want_at(stop, form):
    """What the kit reads at stop k of a layer (0 = the state the layer starts from: the embedding's planes or the previous layer's FFN-2)."""
    x8 = form["x8"]
    stream = STREAM if x8 else ("x16", "xlo")
    w = {0: stream + ("lnstats",),
         1: ("qkv",) + (("vlo_sp",) if x8 and not form["two_plane"] else ()),
         3: stream + ("lnpart", "ctx") + (("ctx8",) if x8 else ()) + (("cls_lo768",) if form["cls_as"] else ()),
         4: ("h16",) + (("h8",) if x8 else ()) + (("cls_lo3072",) if form["cls_as"] else ()),
         5: stream + ("lnstats",)}[stop]
    if stop == 1 and form["tile_both"] is not None:
        w = w + ("tile_both",)
    return w


def layer_records(states, form):
    """states {0, 1, 3, 4, 5: read_state(...)} of one layer -> the four launch records.  The pass is deterministic (tests/test_pass_fingerprint_gpu.py pins its
    bits), so the stream a residual GEMM overwrote in place is read from the run stopped before it."""
    x8 = form["x8"]
    s0, s1, s3, s4, s5 = (states[k] for k in (0, 1, 3, 4, 5))
    a_x = lambda st: dict(a_hi=st["x16"], **(dict(a_hi8=st["x_hi8"], a_lo8=st["x_lo8"], a_sp=st["st_lo"]) if x8 else {}))  # noqa: E731
    qkv = dict(a_x(s0), stats=s0["lnstats"], **{k: s1[k] for k in ("q", "k", "v", "q_lo", "k_lo", "v_lo", "vlo_sp") if k in s1})
    out = dict(a_hi=s3["ctx"], stats=s0["lnstats"], stats_out=s3["lnpart"], **stream_rec(s0, form, "s_"), **stream_rec(s3, form, ""))
    if x8:
        out.update(a_hi8=s3["ctx_hi8"], a_lo8=s3["ctx_lo8"], a_sp=s3.get("cls_lo768"))
    f1 = dict(a_x(s3), stats=s3["lnpart"], hi=s4["h16"])
    if x8:
        f1.update(hi8=s4["h_hi8"], lo8=s4["h_lo8"], sp=s4.get("cls_lo3072"))
    f2 = dict(a_hi=s4["h16"], stats=s3["lnpart"], stats_out=s5["lnstats"], **stream_rec(s3, form, "s_"), **stream_rec(s5, form, ""))
    if x8:
        f2.update(a_hi8=s4["h_hi8"], a_lo8=s4["h_lo8"], a_sp=s4.get("cls_lo3072"))
    return dict(qkv=qkv, out_proj=out, ffn1=f1, ffn2=f2)


def check_layer(recs, lw, form, lens, rep=None):
    """All four launches of a layer; returns (Report, the modelled activations: for the x8_sat check)."""
    rep = rep or Report()
    m_qkv = check_qkv(rep, recs["qkv"], lw, form, lens)
    m_o = check_residual(rep, "out_proj", recs["out_proj"], lw["wo"], lw["bo"], lw["pend_g"], lw["pend_b"], form, lens)
    _, m_h = check_ffn1(rep, recs["ffn1"], lw, form, lens)
    m_2 = check_residual(rep, "ffn2", recs["ffn2"], lw["w2"], lw["b2"], lw["ln1g"], lw["ln1b"], form, lens)
    real = np.arange(m_o.shape[1])[None, :] < np.asarray(lens)[:, None]
    # every activation that gets fp8 planes: the stream the layer reads and the context (engine values: their producers are the embedding and attention
    # kernels), the modelled outputs of the output projection, FFN-1 and FFN-2
    amax = max(float(np.abs(x[real]).max()) for x in (m_o, m_h, m_2, stream64(recs["out_proj"], lens, form), recs["out_proj"]["a_hi"]))
    return rep, dict(qkv=m_qkv, act_max=amax)


# ---- numpy emulation of the launches: float32 accumulation K-tile by K-tile, then the storage roundings ----------------------------------------------------------------

# "hi8_only_in_tile_both" is the issue's "hi8 plane written where out8_hi_only should have kept a special block's lo8 row", restated for the kernel as it is:
# gemm_pp.h decides  hi_only = out8_hi_only && !tile_short  per row TILE (no 32-row block keeps a lo8 row any more: the special rows' low parts travel through
# sp_lo_out; the header comment of gemm_pp.h that speaks of such a block predates that), so the lo8 plane that has to be kept is a tile_both tile's.
MUTATIONS = ("cls_row_term_dropped", "sep_row_term_dropped", "row_term_twice", "wside_dropped", "aside_missing_tile_both", "prev_tile_stats",
             "stats_two_of_three", "vstats_after_store", "lo8_neighbour_block", "hi8_only_in_tile_both", "vt_not_transposed", "col0_ignored")
_f32, _f16 = np.float32, np.float16
MFMA_SPLIT = ROUNDINGS_PER_MFMA  # roundings of the accumulator per MFMA instruction in the emulation: what the engine shows (allowance())


def _mm32(a, w, step, acc0=None):
    """a [M, K] x w [N, K]^T into float32 accumulators that start from acc0 (the kernel's accumulators hold bias + LayerNorm(residual) before the first
    MFMA), `step` K-elements — one rounding of the accumulators: 32 / MFMA_SPLIT of the fp16 sweep (16x16x32), 128 / MFMA_SPLIT of the fp8 sweep (16x16x128) — at a time."""
    acc = np.zeros((a.shape[0], w.shape[0]), _f32) if acc0 is None else acc0.astype(_f32).copy()
    for k in range(0, a.shape[1], step):
        acc += a[:, k:k + step].astype(_f32) @ w[:, k:k + step].astype(_f32).T
    return acc


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_f32)


def _ln32(stats, two_of_three=False):
    """common.h ln_from_partials in float32 (the hardware reciprocal square root taken as correctly rounded)."""
    s = np.asarray(stats, _f32)
    if two_of_three:
        s1, s2 = s[..., 0, 0] + s[..., 1, 0], s[..., 0, 1] + s[..., 1, 1]
    else:
        s1, s2 = (s[..., 0, 0] + s[..., 1, 0]) + s[..., 2, 0], (s[..., 0, 1] + s[..., 1, 1]) + s[..., 2, 1]
    mean = s1 * _f32(1.0 / H)
    var = np.maximum(s2 * _f32(1.0 / H) - mean * mean, _f32(0))
    return mean[..., None], (1.0 / np.sqrt((var + _f32(LN_EPS)).astype(np.float64))).astype(_f32)[..., None]


def _sweeps32(rec, Wm, form, lens, aside, init, mutation, row_term=True):
    """The accumulators of a launch after its sweeps and the special rows' row term.  aside: bool [B, Sp, N or 1], where the A-side term is swept; the special
    rows take the row term where it is not (and rec["a_sp"] is there)."""
    B, Sp, K = rec["a_hi"].shape
    N = Wm.shape[0]
    flat = lambda x: x.reshape(B * Sp, -1)  # noqa: E731
    if not form["x8"]:
        return _mm32(flat(rec["a_hi"]), pm._f16(Wm), 32 // MFMA_SPLIT, init).reshape(B, Sp, N)
    wh, wh8, wl8 = pm._w_planes(Wm)
    acc = _mm32(flat(rec["a_hi"]), wh, 32 // MFMA_SPLIT, init)
    if mutation != "wside_dropped":
        acc = _mm32(flat(rec["a_hi8"]), wl8, 128 // MFMA_SPLIT, acc)
    aside = np.broadcast_to(aside, (B, Sp, N))
    if aside.any():
        acc = np.where(flat(aside), _mm32(flat(np.nan_to_num(rec["a_lo8"])), wh8, 128 // MFMA_SPLIT, acc), acc)
    acc = acc.reshape(B, Sp, N).copy()
    if row_term and rec.get("a_sp") is not None:
        rows = special_rows(lens)
        for j in (0, 1):
            if mutation == ("cls_row_term_dropped", "sep_row_term_dropped")[j]:
                continue
            corr = _mm32(rec["a_sp"][:, j], wh, 32)  # the skinny fp16 GEMM in front of the launch: fp32 [B, N], 2^11 x the term
            for b in range(B):
                r = rows[b, j]
                take = ~aside[b, r] if mutation != "row_term_twice" else np.ones(N, bool)
                acc[b, r] = np.where(take, _fma32(corr[b], 1.0 / 2048.0, acc[b, r]), acc[b, r])
    return acc


def _prev_tile(x, axis, n=256):
    return np.roll(x, n, axis=axis)


def emulate_qkv(rec, lw, form, lens, mutation=None, col0=0):
    """PP_QK.  col0 = 768: the K / V-only launch of the pruned last layer (outputs k, v only)."""
    B, Sp, _ = rec["a_hi"].shape
    Wm, bias = lw["wqkv"][col0:], lw["bqkv"][col0:]
    N = Wm.shape[0]
    blk = (np.arange(N) + (0 if mutation == "col0_ignored" else col0)) // H
    aside = np.broadcast_to((((form["qkv_mask"] >> blk) & 1) == 1)[None, None, :], (B, Sp, N)) if form["x8"] else np.zeros((B, Sp, 1), bool)
    acc = _sweeps32(rec, Wm, form, lens, aside, np.zeros((B * Sp, N), _f32), mutation, row_term=form["x8"] and form["qkv_mask"] != 7)
    _, rstd = _ln32(rec["stats"], mutation == "stats_two_of_three")
    bp = bias.astype(_f32)
    if mutation == "prev_tile_stats":
        rstd, bp = _prev_tile(rstd.reshape(B * Sp, 1), 0).reshape(B, Sp, 1), _prev_tile(bp, 0)
    v = _fma32(rstd, acc, bp)
    hi = v.astype(_f16)
    lo = (v - hi.astype(_f32)).astype(_f16)
    out = {}
    names = "qkv"[col0 // H:]
    if mutation == "col0_ignored":  # the block index taken without col0: K lands in Q's buffer, V (untransposed) in K's, nothing in V^T's
        names = "qk"
        out["v"] = np.zeros((B, Sp, H))
        out["v_lo"] = np.zeros((B, Sp, H))
        if col0:
            out["k"] = np.zeros((B, Sp, H))
            out["k_lo"] = np.zeros((B, Sp, H))
    for i, nm in enumerate(names):
        out[nm], out[nm + "_lo"] = hi[..., i * H:(i + 1) * H].astype(np.float64), lo[..., i * H:(i + 1) * H].astype(np.float64)
    if mutation == "vt_not_transposed":  # a 64 token x 64 dim tile of a head stored as it lies in the accumulators
        for nm in ("v", "v_lo"):
            t = out[nm].reshape(B, Sp // 64, 64, HEADS, HD)
            out[nm] = t.transpose(0, 1, 4, 3, 2).reshape(B, Sp, H)
    if not form["two_plane"]:
        for nm in "qkv":
            out.pop(nm + "_lo", None)
        if form["x8"] and "v" in names:
            i = names.index("v")
            out["vlo_sp"] = _special_compact(((v - hi.astype(_f32)) * _f32(2048.0)).astype(_f16).astype(np.float64)[..., i * H:(i + 1) * H], lens)
    return out


def _producer_planes(v, form, lens, lo8_rows, mutation, stale=None):
    """The planes of an fp32 result v [B, Sp, N]: hi, (hi8, lo8, sp | lo)."""
    hi = v.astype(_f16)
    low = (v - hi.astype(_f32)).astype(np.float64)
    out = dict(hi=hi.astype(np.float64))
    if not form["x8"]:
        out["lo"] = low.astype(_f16).astype(np.float64)
        return out
    out["hi8"] = pm._e4m3(v.astype(np.float64) * SH) / SH
    lo8 = pm._e4m3(low * (2048.0 * SH)) / (2048.0 * SH)
    if mutation == "lo8_neighbour_block":
        B, Sp, N = v.shape
        lo8 = np.roll(lo8.reshape(B * Sp, N), 32, axis=0).reshape(B, Sp, N)
    out["lo8"] = np.where(lo8_rows[..., None], lo8, 0.0 if stale is None else stale)
    out["sp"] = _special_compact((low * 2048.0).astype(_f16).astype(np.float64), lens)
    return out


def _both_rows(form, lens, Sp, mutation):
    both = form["both"].copy()
    if mutation == "aside_missing_tile_both" and form["cls_as"]:
        both[:] = False
    return np.broadcast_to(both[:, None, None], (len(lens), Sp, 1))


def emulate_residual(rec, Wm, bias, g, b, form, lens, mutation=None):
    """PP_RESLN3: accumulators start from bias + LayerNorm(stream_in) (float32, unfused), the sweeps, the row term, vstats from the accumulators, the planes."""
    B, Sp, _ = rec["a_hi"].shape
    N = Wm.shape[0]
    mean, rstd = _ln32(rec["stats"], mutation == "stats_two_of_three")
    r = stream64(rec, lens, form).astype(_f32)  # hi + the decoded low part: one fp32 addition of two fp16 values
    t = (r - mean) * rstd
    init = _fma32(t, g.astype(_f32), b.astype(_f32)) + bias.astype(_f32)
    aside = _both_rows(form, lens, Sp, mutation)
    has_rt = form["cls_as"] and mutation != "aside_missing_tile_both"
    v = _sweeps32(rec, Wm, form, lens, aside, init.reshape(B * Sp, N), mutation, row_term=has_rt)
    out = _producer_planes(v, form, lens, np.ones((B, Sp), bool), mutation)
    sv = out["hi"].astype(_f32) if mutation == "vstats_after_store" else v
    t3 = sv.reshape(B, Sp, 3, 256)
    out["stats_out"] = np.stack([t3.sum(-1, dtype=_f32), (t3.astype(np.float64) ** 2).sum(-1).astype(_f32)], -1).astype(np.float64)
    return out


def emulate_ffn1(rec, lw, form, lens, mutation=None):
    """PP_GELU: fma(rstd, acc, b'), GELU, the planes of the activated value (lo8 only where out8_hi_only leaves it: rows of a tile_both tile)."""
    B, Sp, _ = rec["a_hi"].shape
    aside = _both_rows(form, lens, Sp, mutation)
    has_rt = form["cls_as"] and mutation != "aside_missing_tile_both"
    acc = _sweeps32(rec, lw["w1"], form, lens, aside, np.zeros((B * Sp, INTER), _f32), mutation, row_term=has_rt)
    _, rstd = _ln32(rec["stats"], mutation == "stats_two_of_three")
    bp = lw["b1"].astype(_f32)
    if mutation == "prev_tile_stats":
        rstd, bp = _prev_tile(rstd.reshape(B * Sp, 1), 0).reshape(B, Sp, 1), _prev_tile(bp, 0)
    v = orc._gelu(_fma32(rstd, acc, bp).astype(np.float64)).astype(_f32)
    lo8_rows = np.broadcast_to(form["both"][:, None], (B, Sp)) if form["cls_as"] else np.ones((B, Sp), bool)
    if mutation == "hi8_only_in_tile_both":
        lo8_rows = np.zeros((B, Sp), bool)
    return _producer_planes(v, form, lens, lo8_rows, mutation)


# ---- synthetic operands for the emulation ------------------------------------------------------------------------------------------------------------------------------

def synth_planes(x, form, lens, pfx):
    """The planes an engine would hold of the unrounded activation x [B, Sp, K], as record fields: pfx "a_" (a GEMM operand) or "s_" (the stream)."""
    hi, hi8, lo8 = pm._x8_planes(x, pm.X8_ACT_SHIFT)
    r = {pfx + "hi": hi}
    if form["x8"]:
        r.update({pfx + "hi8": hi8, pfx + "lo8": lo8, pfx + "sp": _special_compact(pm._f16((x - hi) * 2048.0), lens)})
    elif pfx == "s_":
        r["s_lo"] = pm._f16(x - hi)
    return r


def synth_stats(x):
    """vstats [B, Sp, 3, 2] of a stream x as a producer leaves them: float32 sums of the unrounded rows per 256-column tile."""
    t = x.reshape(x.shape[0], x.shape[1], 3, 256)
    return np.stack([t.sum(-1).astype(_f32), (t ** 2).sum(-1).astype(_f32)], -1).astype(np.float64)


def synth_layer(seed, B, Sp):
    """Random operands with outlier columns (tests/test_gpu_kernels.py) and a peaked-LayerNorm stream: a row mean of several standard deviations and two
    dimensions 20 x the rest; weights at 0.04 with row-centred folded matrices.  Returns (lw, acts) with acts = dict(stream, ctx, h) unrounded [B, Sp, K]."""
    rng = np.random.default_rng(seed)
    col = lambda K: 1.0 + 3.0 * (rng.random((1, 1, K)) < 0.01)  # noqa: E731
    stream = rng.standard_normal((B, Sp, H)) * col(H) + 2.5
    stream[..., [17, 401]] *= 20.0
    ctx = rng.standard_normal((B, Sp, H)) * col(H)
    h = orc._gelu(rng.standard_normal((B, Sp, INTER)) * 1.5 * col(INTER))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    cen = lambda Wm: f32(Wm - Wm.mean(-1, keepdims=True))  # noqa: E731
    Wr = lambda n, k: rng.standard_normal((n, k)) * 0.04  # noqa: E731
    lw = dict(wqkv=cen(Wr(3 * H, H)), bqkv=f32(rng.standard_normal(3 * H) * 0.1), wo=f32(Wr(H, H)), bo=f32(rng.standard_normal(H) * 0.1),
              w1=cen(Wr(INTER, H)), b1=f32(rng.standard_normal(INTER) * 0.1), w2=f32(Wr(H, INTER)), b2=f32(rng.standard_normal(H) * 0.1),
              pend_g=f32(1.0 + 0.1 * rng.standard_normal(H)), pend_b=f32(0.1 * rng.standard_normal(H)),
              ln1g=f32(1.0 + 0.1 * rng.standard_normal(H)), ln1b=f32(0.1 * rng.standard_normal(H)))
    for k in ("pend_g", "ln1g"):  # LayerNorm outlier dimensions: the residual GEMMs' outputs reach ~40 rms there (below the fp8 planes' 112)
        lw[k][[17, 401]] *= 3.0
    return lw, dict(stream=stream, ctx=ctx, h=h)


# ---- which row tiles a workgroup of the persistent grid computes after its first ---------------------------------------------------------------------------------------

def later_row_tiles(M, N, num_cu, gn_max=4):
    """{tile_m} of the 256^2 output tiles a workgroup computes in its second or a later iteration: encoder_pass.h launch_pp (grid = min(tiles, #CUs), GN = the
    largest divisor of N / 256 up to gn_max) and gemm_pp.h raster_pp, mode 0 (logical tile L = it G + slot; column group > tile_m > tile_n in the group)."""
    tm, tn = M // 256, N // 256
    GN = max(d for d in range(1, min(gn_max, tn) + 1) if tn % d == 0)
    G = min(tm * tn, num_cu)
    return {(L % (tm * GN)) // GN for L in range(G, tm * tn)}


def sub_form(form, seqs):
    return dict(form, both=form["both"][np.asarray(seqs)])
