"""Every launch of the reference form (compute dtype "f32": memvul_amd/csrc/ref_f32.h, encoder_pass.h encode_f32_dev) on the engine's own operands: the QKV GEMM,
attention_f32_kernel, the output projection in place on the stream (res == C), LayerNorm 1, FFN-1 with the erf GELU, FFN-2 in place, LayerNorm 2 — element by
element, every row of every sequence and every column for the GEMMs and LayerNorms, every real row, head and dim for attention.

The development build's MEMVUL_DEBUG_STOP=k ends an MV_F32 pass inside its last layer (3: before LayerNorm 1, 4: after LayerNorm 1 and FFN-1, 5: before
LayerNorm 2); with the unstopped engine and the planes 35 (Q | K | V), 36 (context), 37 (GELU output), which a layer writes once, every launch's input and output
is a tap.  The float64 models and the bounds are tests/f32_stage_kit.py's: the GEMM bound of test_gemm_against_float64, cls_tail_kit.ln_model, and for attention
pav x (C_S x u x smag + 8 u) with the chain constant tests/test_f32_stage_cpu.py measures on a numpy emulation of the kernel, where it also shows the faults that
bound catches.  Recorded per launch, layer, model and case (gpu_util.record, f32_stage_*): the share of the bound the worst element needs, and the rms share.
A share above 1 is a finding, not a bound to raise.  Measured on the MI355X (profiles/f32_form_parity.md), the worst element of any case: QKV 0.72, attention 0.72
(0.73 on the sink case), output projection 0.26, LayerNorm 1 0.23, FFN-1 0.87 (outliers2, layer 2), FFN-2 0.13, LayerNorm 2 0.24; rms shares 0.01 - 0.07."""
import os
import time

import numpy as np
import pytest

import cls_tail_kit as ctk
import f32_stage_kit as fsk
import stage_kit as sk

pytestmark = pytest.mark.gpu

L2 = dict(layers=2, vocab_size=2048)
MODELS = {"peaky2": dict(qk_scale=4.0), "outliers2": dict(qk_scale=4.0, ln_outliers=True)}  # the 2-layer models of tests/test_gemm_stage_gpu.py
# name: (padded length, lens): the smallest passes that reach every branch — len % 32 in {0, 1, 31} in the last chunk, one chunk and several, every padded length
PASSES = {
    "s64": (64, (1, 2, 31, 32, 33, 63, 64)),       # M = 448 in Mpad = 512
    "s128": (128, (65, 96, 97, 128)),
    "s192": (192, (129, 160, 192)),
    "s256": (256, (193, 225, 256)),
    "s384": (384, (257, 353, 384)),
    "s512": (512, (385, 481, 512, 1)),
}
STOPS = (3, 4, 5)
LAUNCHES = ("qkv", "attention", "out_proj", "ln1", "ffn1", "ffn2", "ln2")
_owned = {}  # model -> {0 (unstopped), 3, 4, 5: Engine}: the engines of one model stay alive together


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    t0 = time.time()
    yield gpu_util
    _close_owned()
    gpu_util.record("f32_stage_wall", seconds=time.time() - t0)


def _close_owned():
    for engs in _owned.values():
        for e in engs.values():
            e.close()
    _owned.clear()


def _make_engine(gu, model, compute="f32", env=None, dev=True, **kw):
    """One engine with `env` set while mv_create reads its switches, outside gpu_util's cache (which holds two)."""
    from memvul_amd import binding

    dims, w = gu.weights_for(L2, MODELS[model])
    switches = ("MEMVUL_CLS_PRUNE", "MEMVUL_STREAMS", "MEMVUL_QKV_ASIDE", "MEMVUL_CLS_ASIDE", "MEMVUL_CLS_ASIDE_MIN_LEN", "MEMVUL_FORM") + binding.DEV_SWITCHES
    old = {k: os.environ.pop(k, None) for k in switches}
    os.environ.update(env or {})
    try:
        e = binding.Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_pos=dims.max_pos, dev=dev, **dict(dict(max_tokens=2048, max_batch=8, max_anchors=8), **kw))
    finally:
        for k in switches:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    e.load_state_dict(w, compute)
    return e


def _engines(gu, model):
    if model not in _owned:
        _close_owned()
        _owned[model] = {k: _make_engine(gu, model, env={"MEMVUL_DEBUG_STOP": str(k)} if k else {}) for k in (0,) + STOPS}
    return _owned[model]


def _rows(x):
    """[B, Sp, N] fp32 -> float64 [B Sp, N]."""
    return np.asarray(x, np.float64).reshape(-1, x.shape[-1])


def _attention_shares(qkv, ctx, lens):
    """(max, rms) of the share of the attention bound over the real rows, all heads and dims; all of ctx finite."""
    assert np.isfinite(ctx).all()  # the rows past len and the masked keys' p = 0 x V included
    q, k, v = fsk.split_qkv(qkv)
    share, _ = fsk.attention_share(fsk.heads_of(ctx), q, k, v, lens)
    real = share[sk.row_mask(lens, share.shape)]
    return float(real.max()), float(np.sqrt((real ** 2).mean()))


def layer_shares(engs, lw, ids, lens, n, x_in):
    """Layer n (1-based) of the pass launch by launch: {launch: (max share, rms share)}, and the layer's normalised output (the next layer's input).
    x_in: tap 0 of the unstopped engine after n - 1 layers."""
    out = {}

    def put(launch, got, model_bound):
        want, bound = model_bound
        assert np.isfinite(got).all(), launch
        out[launch] = ctk.stats(ctk.share(_rows(got), want, bound))

    e3, e4, e5, e0 = engs[3], engs[4], engs[5], engs[0]
    e3.debug_encode(ids, lens, n)
    qkv, ctx, raw1 = e3.debug_read(35), e3.debug_read(36), e3.debug_read(0)
    put("qkv", qkv, fsk.gemm_model(_rows(x_in), lw["wqkv"], lw["bqkv"], "bias"))
    out["attention"] = _attention_shares(qkv, ctx, lens)
    put("out_proj", raw1, fsk.gemm_model(_rows(ctx), lw["wo"], lw["bo"], "res", res=_rows(x_in)))   # res == C: the stream in place
    e4.debug_encode(ids, lens, n)
    ln1, h = e4.debug_read(0), e4.debug_read(37)
    put("ln1", ln1, ctk.ln_model(_rows(raw1), lw["ln1g"], lw["ln1b"]))
    put("ffn1", h, fsk.gemm_model(_rows(ln1), lw["w1"], lw["b1"], "gelu"))
    e5.debug_encode(ids, lens, n)
    raw2 = e5.debug_read(0)
    put("ffn2", raw2, fsk.gemm_model(_rows(h), lw["w2"], lw["b2"], "res", res=_rows(ln1)))
    e0.debug_encode(ids, lens, n)
    ln2 = e0.debug_read(0)
    put("ln2", ln2, ctk.ln_model(_rows(raw2), lw["ln2g"], lw["ln2b"]))
    return out, ln2


CASES = [(m, p) for m in MODELS for p in PASSES]


@pytest.mark.parametrize("model,name", CASES)
def test_each_launch_of_the_reference_form_on_its_own_operands(gu, model, name):
    Sp, lens = PASSES[name]
    dims, w = gu.weights_for(L2, MODELS[model])
    ids, lens = sk.boundary_ids(Sp, lens, dims.vocab_size, seed=7)
    engs = _engines(gu, model)
    t0 = time.time()
    engs[0].debug_encode(ids, lens, 0)
    x = engs[0].debug_read(0)  # layer 1 reads the embedding kernel's stream, layer 2 a LayerNorm's over a residual GEMM's
    bad, worst = [], 0.0
    for n in (1, 2):
        shares, x = layer_shares(engs, fsk.layer_weights(w, n - 1), ids, lens, n, x)
        assert set(shares) == set(LAUNCHES)
        for launch in LAUNCHES:
            mx, rms = shares[launch]
            print(f"f32 {model} {name} layer {n} {launch}: max share {mx:.3f} rms share {rms:.3f}")
            gu.record("f32_stage_parity", launch=launch, layer=n, model=model, case=name, max_share=mx, rms_share=rms)
            worst = max(worst, mx)
            if not mx <= 1.0:
                bad.append((n, launch, mx))
    gu.record("f32_stage_case", model=model, case=name, seconds=time.time() - t0, worst=worst)
    assert not bad, bad


def test_attention_on_an_ordinary_token_sink(gu, golden_dir):
    """mid_all_80_3001 of tests/golden/r06_sink_refs.npz — 80 % of every row's mass on one ordinary token, the largest score spread the project has committed —
    through the product library: attention alone, at layers 1 and 12."""
    import test_safe_form_gpu as tsf
    from memvul_amd.binding import Engine

    case = "mid_all_80_3001"
    refs = np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))
    dims, w, ids, lens, _, _ = tsf._sink_case(refs, case)
    _close_owned()
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=ids.shape[0] * sk.padded_len(ids.shape[1]), max_batch=16, max_anchors=16)
    try:
        eng.load_state_dict(w, "f32")
        bad = []
        for n in (1, dims.layers):
            eng.debug_encode(ids, lens, n)
            qkv, ctx = eng.debug_read(35), eng.debug_read(36)
            q, k, _ = fsk.split_qkv(qkv)
            spread = max(float((q[b, :, :m] @ k[b, :, :m].transpose(0, 2, 1)).std(-1).max()) for b, m in enumerate(lens))
            mx, rms = _attention_shares(qkv, ctx, lens)
            print(f"f32 {case} layer {n} attention: max share {mx:.3f} rms share {rms:.3f} (largest score std of a row {spread:.1f})")
            gu.record("f32_stage_sink", case=case, layer=n, launch="attention", max_share=mx, rms_share=rms, score_std_max=spread)
            if not mx <= 1.0:
                bad.append((n, mx))
        assert not bad, bad
    finally:
        eng.close()


def test_taps_and_stops(gu):
    Sp, lens = PASSES["s64"]
    dims, _ = gu.weights_for(L2, MODELS["peaky2"])
    ids, lens = sk.boundary_ids(Sp, lens, dims.vocab_size, seed=7)
    # the fp32 planes do not exist on a handle of another compute dtype
    for compute in ("precise", "f16"):
        e = _make_engine(gu, "peaky2", compute=compute, dev=False)
        try:
            e.debug_encode(ids, lens, 1)
            for tap in (35, 36, 37):
                with pytest.raises(RuntimeError, match="does not exist in this compute dtype"):
                    e.debug_read(tap)
        finally:
            e.close()
    engs = _engines(gu, "peaky2")
    e0 = engs[0]
    # the product library does not read the stop: the pass runs to its end, and its bits are the unstopped development engine's
    prod = _make_engine(gu, "peaky2", env={"MEMVUL_DEBUG_STOP": "3"}, dev=False)
    try:
        for n in (0, 2):
            prod.debug_encode(ids, lens, n)
            e0.debug_encode(ids, lens, n)
            for tap in (0, 10) + ((35, 36, 37) if n else ()):
                assert prod.debug_read(tap).tobytes() == e0.debug_read(tap).tobytes(), (n, tap)
        assert prod.encode(ids, lens).tobytes() == e0.encode(ids, lens).tobytes()
        for tap in (1, 5, 9):  # the fp16 planes still refuse
            with pytest.raises(RuntimeError, match="fp16"):
                prod.debug_read(tap)
    finally:
        prod.close()
    # stops 1 and 2 leave the stream as layer 2 found it; the planes they wrote are the ones the later stops show
    e0.debug_encode(ids, lens, 1)
    x1 = e0.debug_read(0)
    engs[3].debug_encode(ids, lens, 2)
    qkv, ctx = engs[3].debug_read(35), engs[3].debug_read(36)
    for k, tap, want in ((1, 35, qkv), (2, 36, ctx)):
        e = _make_engine(gu, "peaky2", env={"MEMVUL_DEBUG_STOP": str(k)})
        try:
            e.debug_encode(ids, lens, 2)
            assert e.debug_read(0).tobytes() == x1.tobytes(), k
            assert e.debug_read(tap).tobytes() == want.tobytes(), k
        finally:
            e.close()
    # a stop with no layers: the embedding kernel's stream as it is
    e0.debug_encode(ids, lens, 0)
    emb = e0.debug_read(0)
    for k in STOPS:
        engs[k].debug_encode(ids, lens, 0)
        assert engs[k].debug_read(0).tobytes() == emb.tobytes(), k
    # a stopped engine's ordinary forward is untouched: only mv_debug_encode carries the stop
    assert engs[3].encode(ids, lens).tobytes() == e0.encode(ids, lens).tobytes()
