"""Attention and the per-layer stream on the engine's own operands, row by row (the end-to-end tests read token 0 of a sequence: every other row reaches the
pooler averaged over the attention keys, so a defect in one key, one row of a tile or one chunk boundary is diluted by ~ 1 / len in the logits).

1. Attention against float64 (tests/stage_kit.py).  After debug_encode(ids, lens, n) the Q, K, V^T planes layer n's attention read (taps 2 - 4, and their low
   planes 7 - 9 where the pass wrote them) go through softmax(q k^T + additive -10000 mask) v in float64, and the context the kernel wrote (tap 5) is held to a
   bound DERIVED from the roundings the kernel performs (stage_kit.bound_two_plane / bound_one_plane), element by element, on every query row < len, all 12
   heads, all 64 dims, every layer of the model — nothing sampled.  Engines: the default form of MV_F16X8 (one-plane attention_v2_kernel<NKB, NCH, 1, 0> with
   its special-row V term above 128 keys, the two-plane <1, 1> / <2, 1> short passes up to 128), its safe form (two planes at every length) and MV_F16
   (<NKB, NCH, 0>).  Passes: one batch per padded length with its rows ON the edges of the key mask and of the chunks (stage_kit.BOUNDARY_BATCHES), the item-loop
   shapes (more units than resident workgroups, neighbouring units of different lengths: the O tile of one unit is written out during the next), and an
   ordinary-token attention sink (P ~ 0.8 on one key).  tests/test_stage_parity_cpu.py shows without a GPU that a numpy emulation of the kernel stays at 0.4 -
   0.9 of these bounds and that an unmasked key, a skipped chunk rescale, a tile written to its neighbour's rows or a permutation applied to V alone leave
   them by a factor of 100 to 10 000.
2. Every row of every layer's normalised stream (tap 0) against the float64 oracle, scaled by the precision model (oracle/precision_model.py): the rms error of
   an engine row may not exceed K = 2 times the 99th percentile of the MODEL's row errors in that layer.  The bound comes from the model, never from the engine.

Measured on the MI355X: profiles/stage_parity.md."""
import os
import sys
import time

import numpy as np
import pytest

from memvul_amd import synth

import stage_kit as sk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ENGINES = ("precise", "safe", "f16")
L2 = dict(layers=2, vocab_size=2048)
WK = dict(qk_scale=4.0)  # the peaked 2-layer model of tests/test_gpu_kernels.py


def _trained():
    """The 12-layer trained-like model (LayerNorm outlier dims, peaked attention, matcher x29: scripts/r06_make_sink_refs.py KW on the envelope seed)."""
    import r05_make_refs as mk5
    import r06_make_sink_refs as mk6

    return dict(layers=12), dict(seed=mk5.ENV_SEED, **mk6.KW)


def _model(name):
    return (L2, WK) if name == "peaky2" else _trained()


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    t0 = time.time()
    yield gpu_util
    gpu_util.record("stage_parity_wall", seconds=time.time() - t0)


def _check_layers(gu, eng, engine, model, case, ids, lens, layers):
    """Part 1 for one pass: every layer of `layers`, recorded one by one, all of them asserted."""
    worst = {}
    for n in layers:
        mx, rms = sk.attention_ratio(eng, engine, ids, lens, n)
        worst[n] = mx
        gu.record("stage_parity_attention", engine=engine, model=model, case=case, layer=n, two_plane=bool(sk.two_plane(engine, sk.padded_len(ids.shape[1]))),
                  max_ratio=mx, rms_ratio=rms)
    print(f"{engine} {model} {case}: max |ctx - float64| / bound by layer {({n: round(v, 3) for n, v in worst.items()})}")
    assert max(worst.values()) <= 1.0, worst


# ---- 1. attention on the engine's own operands ---------------------------------------------------------------------------------------------------------------------

BOUNDARY_CASES = [(e, m, b) for e in ENGINES for m in ("peaky2", "trained12") for b in sk.BOUNDARY_BATCHES]


@pytest.mark.parametrize("engine,model,batch", BOUNDARY_CASES, ids=lambda v: sk.batch_id(v) if isinstance(v, tuple) else v)
def test_attention_at_the_length_boundaries(gu, engine, model, batch):
    """Rows whose lengths sit on both sides of every edge the key mask and the chunk loop have (thr = len - j S - 8 hi; chunks wholly past len still rescale O),
    every layer of the model."""
    dk, wk = _model(model)
    dims, _ = gu.weights_for(dk, wk)
    Sp, width, lens = batch
    ids, lens = sk.boundary_ids(width, lens, dims.vocab_size)
    assert sk.padded_len(width) == Sp
    eng = gu.engine_for(dk, wk, compute_dtype=engine)
    assert eng.form == ("safe" if engine == "safe" else "default")
    _check_layers(gu, eng, engine, model, sk.batch_id(batch), ids, lens, range(1, dims.layers + 1))


ITEM_CASES = [(e, m, n, B, S) for e in ENGINES for m, n in (("peaky2", 1), ("trained12", 6)) for B, S in sk.ITEM_LOOP_SHAPES]


@pytest.mark.parametrize("engine,model,layer,B,S", ITEM_CASES)
def test_attention_item_loop_on_the_engines_own_operands(gu, engine, model, layer, B, S):
    """The shapes of tests/test_gpu_kernels.py test_attention_persistent_item_loop: more units than resident workgroups, ragged lengths — the normalised O tile
    of a unit is written out during the NEXT unit of the workgroup, which has another length."""
    dk, wk = _model(model)
    dims, _ = gu.weights_for(dk, wk)
    ids, lens = synth.make_ids(B, S, dims.vocab_size, ragged=True)
    eng = gu.engine_for(dk, wk, compute_dtype=engine, max_batch=70)
    _check_layers(gu, eng, engine, model, f"items_{B}x{S}", ids, lens, [layer])


@pytest.mark.parametrize("engine", ENGINES)
def test_attention_under_an_ordinary_token_sink(gu, golden_dir, engine):
    """mid_all_80_3001 (tests/golden/r06_sink_refs.npz): every head of every layer puts ~ 0.8 of every row's mass on one ordinary token — one key carries the
    row, its V reaches the context un-averaged.  Its own 8 x 256 inputs, every layer."""
    import r06_make_sink_refs as mk6
    from memvul_amd.binding import Engine

    refs = np.load(os.path.join(golden_dir, "r06_sink_refs.npz"))
    dims, w, ids, lens = mk6.case("mid", "all", 0.80, 3001, gains=refs["mid_all_80_3001_gains"])[:4]
    assert ids.shape == (8, 256)
    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=16 * 512, max_batch=16, max_anchors=16)
    try:
        eng.load_state_dict(w, engine)
        _check_layers(gu, eng, engine, "sink_mid_all_80_3001", "own_8x256", ids, lens, range(1, 13))
    finally:
        eng.close()


# ---- 2. every row of every layer against the float64 oracle, scaled by the precision model --------------------------------------------------------------------------

# the model is one draw of the rounding noise, the engine another; the project's own records have them tens of percent apart on medians (README: +14 % modelled,
# +28 % measured).  The bound comes from the model, never from the engine.
K_MODEL = 2.0
_oracle = {}


def _stream_models(gu, name, S):
    """(ids, lens, mask, exact taps, {engine: model taps}) of one ragged batch: the float64 forward without roundings and with each engine's."""
    from oracle import precision_model as pm

    if (name, S) not in _oracle:
        dk, wk = (dict(layers=12), _trained()[1]) if name == "trained12" else (L2, dict(qk_scale=4.0, ln_outliers=True))
        dims, w = gu.weights_for(dk, wk)
        B = {64: 8, 256: 4, 512: 3}[S]
        ids, lens = synth.make_ids(B, S, dims.vocab_size, seed=synth.SEED + 31, ragged=True)
        mask = synth.mask_from_lens(lens, S)
        taps = {"exact": {}, "precise": {}, "f16": {}}
        i64 = ids.astype(np.int64)
        pm.encode(w, i64, mask, None, taps=taps["exact"])
        pm.encode(w, i64, mask, pm.engine_formats(dims.layers, "f16", **pm.X8_ENGINE_SHIPPED), taps=taps["precise"], **pm.SHIPPED_KW)
        pm.encode(w, i64, mask, pm.engine_formats(dims.layers, "f16"), fold_ln=True, taps=taps["f16"])  # the persistent path: LayerNorm folded, two-plane stream
        if len(_oracle) >= 2:
            _oracle.pop(next(iter(_oracle)))
        _oracle[(name, S)] = (dk, wk, dims, ids, lens, mask, taps)
    return _oracle[(name, S)]


STREAM_CASES = [(m, S, e) for m in ("trained12", "outliers2") for S in (64, 256, 512) for e in ("precise", "f16")]


@pytest.mark.parametrize("model,S,engine", STREAM_CASES)
def test_every_row_of_every_layer_within_the_precision_model(gu, model, S, engine):
    """e_eng = rms(tap 0 - exact) of every real row after n layers against K_MODEL x the 99th percentile of e_mod = rms(model - exact) over the real rows of
    that layer — `precise`: X8_ENGINE_SHIPPED with SHIPPED_KW; `f16` forced onto the persistent path (gemm_tile = 512, LayerNorm folded)."""
    dk, wk, dims, ids, lens, mask, taps = _stream_models(gu, model, S)
    eng = gu.engine_for(dk, wk, compute_dtype=engine, **(dict(gemm_tile=512) if engine == "f16" else {}))
    rms = lambda x: np.sqrt((x ** 2).mean(-1))  # noqa: E731
    worst = {}
    for n in range(1, dims.layers + 1):
        eng.debug_encode(ids, lens, n)
        tap = eng.debug_read(0)[:, :S].astype(np.float64)
        e_eng = rms(tap - taps["exact"][n])[mask]
        e_mod = rms(taps[engine][n] - taps["exact"][n])[mask]
        p99 = float(np.percentile(e_mod, 99))
        ratio = e_eng / e_mod
        worst[n] = float(e_eng.max() / p99)
        gu.record("stage_parity_stream", engine=engine, model=model, S=S, layer=n, rows=int(mask.sum()), max_eng_over_mod=float(ratio.max()),
                  median_eng_over_mod=float(np.median(ratio)), max_eng_over_p99_mod=worst[n], p99_mod=p99, max_eng=float(e_eng.max()))
    print(f"{engine} {model} S {S}: max e_eng / p99(e_mod) by layer {({n: round(v, 3) for n, v in worst.items()})}")
    assert max(worst.values()) <= K_MODEL, worst
