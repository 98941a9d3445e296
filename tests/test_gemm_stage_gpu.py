"""Each persistent GEMM launch of a layer on the engine's own operands (tests/gemm_stage_kit.py): QKV projection, output projection, FFN-1, FFN-2 with their row
terms, fp8 planes, virtual LayerNorm statistics and special-row buffers, element by element, every real row and every column.

The development build's MEMVUL_DEBUG_STOP=k ends mv_debug_encode after the first k launch groups of its last layer without the final LayerNorm, so every plane
is what that launch left; the stream a residual GEMM overwrote in place is read from the run stopped before it (the pass is deterministic:
tests/test_pass_fingerprint_gpu.py).  A launch's float64 model is formed from THESE planes (oracle/precision_model.py _mm_planes) and the weights as weights.h
folds them; which rows take which form comes from the documented rule (gsk.pass_form), and the tile_both tap has to equal it (cls_tile_flags_kernel).

Bounds: gemm_stage_kit's — storage rounding + allowance (3e-5 x rms(pre-activation) + the per-MFMA-step fp32 rounding of the element); tests/test_gemm_stage_cpu.py fixes them on a numpy emulation and shows the faults
they catch.  Reported per launch, layer and row class (special rows, both-terms rows, weight-side-only rows): the share of the allowance the worst element
needs, and the rms.  Rows past a sequence's length need only be finite (the rows past B x Sp of a pass are not readable through the taps).
Measured on the MI355X (profiles/gemm_stage_parity.md): the default form on peaky2 needs 0.05 - 0.23 of 3e-5 x rms in every launch and row class; on outliers2
at 64 keys one special-row element of layer 2's FFN-2 needed 1.09 of it (0.81 in layer 1) — the per-step rounding of a residual accumulator that holds an
element of 27 rms: gsk.allowance states it, for the residual GEMMs alone, with the rounding count the engine shows."""
import time

import numpy as np
import pytest

import gemm_stage_kit as gsk
import stage_kit as sk

pytestmark = pytest.mark.gpu

L2 = dict(layers=2, vocab_size=2048)
MODELS = {"peaky2": dict(qk_scale=4.0), "outliers2": dict(qk_scale=4.0, ln_outliers=True)}  # the peaked 2-layer model of tests/test_gpu_kernels.py, and with LayerNorm outlier dims
# name: (kit engine, compute dtype, engine_for keywords, environment, pass_form keywords)
ENGINES = {
    "precise": ("precise", "precise", {}, {}, {}),
    "precise_cls_aside0": ("precise", "precise", {}, {"MEMVUL_CLS_ASIDE": "0"}, dict(cls_aside=False)),
    "precise_qkv_aside_q": ("precise", "precise", {}, {"MEMVUL_QKV_ASIDE": "q"}, dict(qkv_aside="q")),
    "safe": ("safe", "safe", {}, {}, {}),
    "f16_tile512": ("f16", "f16", dict(gemm_tile=512), {}, {}),
}
# name: (padded length, lengths): the smallest passes that reach every branch; the first and the last row of a 256-row tile are real rows where a length allows it
PASSES = {
    "s64": (64, (3, 16, 63, 64, 64)),              # M = 320, Mpad = 512: pad rows; lo planes of Q, K, V^T
    "s128": (128, (128, 70)),
    "s192_whole": (192, (192, 128, 150, 191)),     # the whole-pass form; a 256-row tile spans two sequences
    "s192_mixed": (192, (192, 100, 150, 191)),     # one sequence below MEMVUL_CLS_ASIDE_MIN_LEN: the whole-pass form is off
    "s256": (256, (256, 130, 40)),                 # two [CLS]-form tiles and one tile_both tile in one launch
    "s384": (384, (384, 257)),
    "s512": (512, (512, 127)),                     # a sequence of two row tiles, and one flagged in both of its tiles
}
STOPS = (1, 3, 4, 5)
_owned = {}  # (engine, model) -> {stop: Engine}: the four stopped engines of one configuration stay alive together (gpu_util's cache holds two)


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    t0 = time.time()
    yield gpu_util
    for engs in _owned.values():
        for e in engs.values():
            e.close()
    _owned.clear()
    gpu_util.record("gemm_stage_parity_wall", seconds=time.time() - t0)


def _make_engine(gu, model, compute, env, gemm_tile=0, **kw):
    """One development-build engine with `env` set while mv_create reads its switches (what gpu_util.engine_for does, without its cache: the four stopped
    engines of a configuration live together here and evict nobody else's)."""
    import os

    from memvul_amd import binding

    env = dict(env, **({"MEMVUL_GEMM_TILE": str(gemm_tile)} if gemm_tile else {}))
    dims, w = gu.weights_for(L2, MODELS[model])
    switches = ("MEMVUL_CLS_PRUNE", "MEMVUL_STREAMS", "MEMVUL_QKV_ASIDE", "MEMVUL_CLS_ASIDE", "MEMVUL_CLS_ASIDE_MIN_LEN", "MEMVUL_FORM") + binding.DEV_SWITCHES
    old = {k: os.environ.pop(k, None) for k in switches}
    os.environ.update(env)
    try:
        e = binding.Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_pos=dims.max_pos, dev=True, **kw)
    finally:
        for k in switches:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    e.load_state_dict(w, compute)
    return e


def _stopped_engines(gu, engine, model, env_extra=(), **eng_kw):
    key = (engine, model, tuple(env_extra), tuple(sorted(eng_kw.items())))
    if key not in _owned:
        for engs in _owned.values():
            for e in engs.values():
                e.close()
        _owned.clear()
        _, compute, kw, env, _ = ENGINES[engine]
        kw = dict(dict(max_tokens=2048, max_batch=8, max_anchors=8), **kw, **eng_kw)
        _owned[key] = {k: _make_engine(gu, model, compute, dict(env, MEMVUL_DEBUG_STOP=str(k), **dict(env_extra)), **kw) for k in STOPS}
    return _owned[key]


def layer_states(engs, form, ids, lens, n, subsets=((None, None),)):
    """The states 0, 1, 3, 4, 5 of layer n (1-based) of the pass: one dict per (seqs, tokens) subset of `subsets` (gsk.read_state)."""
    out = [dict() for _ in subsets]

    def read(eng, k):
        for st, (seqs, tokens) in zip(out, subsets):
            st[k] = gsk.read_state(eng, form, gsk.want_at(k, form), seqs, tokens)

    if n == 1:
        engs[1].debug_encode(ids, lens, 0)
    else:
        engs[5].debug_encode(ids, lens, n - 1)
    read(engs[1] if n == 1 else engs[5], 0)
    for k in STOPS:
        engs[k].debug_encode(ids, lens, n)
        read(engs[k], k)
    return out if len(out) > 1 else out[0]


def _record(gu, rep, **tags):
    for (launch, cls), (mx, rms) in sorted(rep.by_launch_class().items()):
        gu.record("gemm_stage_parity", launch=launch, row_class=cls, max_ratio=mx, rms_ratio=rms, **tags)
    for (launch, cls), (mx, rms) in sorted(rep.by_launch_class(rounding_only=True).items()):  # hi8, |lo|, vstats: bounds that are a rounding alone
        gu.record("gemm_stage_parity_rounding", launch=launch, row_class=cls, max_ratio=mx, rms_ratio=rms, **tags)
    for launch in ("out_proj", "ffn2"):  # the vstats bound is statistical (6 sigma): its margin on the engine's side
        gu.record("gemm_stage_parity_vstats", launch=launch, max_ratio=max(rep.worst(launch=launch, what="vstats_sum"), rep.worst(launch=launch, what="vstats_sumsq")), **tags)


CASES = [(e, m, p) for e in ENGINES for m in MODELS for p in PASSES]


@pytest.mark.parametrize("engine,model,name", CASES)
def test_each_gemm_launch_on_its_own_operands(gu, engine, model, name):
    kit_engine, _, _, _, form_kw = ENGINES[engine]
    Sp, lens = PASSES[name]
    dims, w = gu.weights_for(L2, MODELS[model])
    ids, lens = sk.boundary_ids(Sp, lens, dims.vocab_size, seed=7)
    form = gsk.pass_form(kit_engine, Sp, lens, **form_kw)
    engs = _stopped_engines(gu, engine, model)
    t0 = time.time()
    worst = {}
    for n in (1, 2):  # layer 1 reads the embedding kernel's planes, layer 2 a residual GEMM's
        states = layer_states(engs, form, ids, lens, n)
        if form["tile_both"] is not None:  # cls_tile_flags_kernel against the documented rule
            assert np.array_equal(states[1]["tile_both"], form["tile_both"]), (states[1]["tile_both"], form["tile_both"])
        recs = gsk.layer_records(states, form)
        for launch, rec in recs.items():  # rows past a sequence's length: finite in every plane the launch wrote
            for k, v in rec.items():
                if v is not None and k not in ("a_lo8", "lo8"):  # (a lo8 plane is not written in every form: what it holds elsewhere is whatever was there)
                    assert np.isfinite(v).all(), (launch, k)
        rep, info = gsk.check_layer(recs, gsk.layer_weights(w, n - 1), form, lens)
        # a clamped element of the fp8 planes would set engine and model apart for a reason no bound covers: the modelled activations stay below 112
        assert info["act_max"] < 112.0, info["act_max"]
        _record(gu, rep, engine=engine, model=model, case=name, layer=n)
        for r in rep.rows:
            print(f"{engine} {model} {name} layer {n} {r['launch']} {r['what']} {r['cls']}: max {r['max_ratio']:.3f} rms {r['rms_ratio']:.3f} (max err {r['max_err']:.3g})")
        worst[n] = rep.worst()
        bad = [r for r in rep.rows if r["max_ratio"] > 1.0]
        assert not bad, bad
    if form["x8"]:
        assert engs[5].x8_saturation() == 0
    gu.record("gemm_stage_parity_case", engine=engine, model=model, case=name, seconds=time.time() - t0, worst=max(worst.values()))


@pytest.mark.parametrize("engine", list(ENGINES))
def test_rows_past_the_last_token_of_a_pass_stay_finite(gu, engine):
    """64 keys, B = 5: M = 320 tokens in Mpad = 512 rows.  The persistent GEMMs compute rows 320 .. 511 like any other; no token lives there and no bound applies,
    but what the launches of a layer leave there — the stream's planes and both vstats, the context's and the GELU output's fp8 planes — has to be finite: the
    row class "pad".  Read from the engine that ends after WHOLE layers (stop 5): the embedding kernel does not touch these rows, so they carry the stream of
    the pass before, and an engine that ended a pass between a residual GEMM and the launch that writes the matching vstats pairs a stream with statistics of
    another (zero statistics under a non-zero row: rstd = 1e6, the fp16 stream overflows — seen on the engines stopped after the output projection; rows no
    launch reads for a token, and a state only the stop switch produces)."""
    kit_engine, _, _, _, form_kw = ENGINES[engine]
    Sp, lens = PASSES["s64"]
    dims, _ = gu.weights_for(L2, MODELS["peaky2"])
    ids, lens = sk.boundary_ids(Sp, lens, dims.vocab_size, seed=7)
    form = gsk.pass_form(kit_engine, Sp, lens, **form_kw)
    eng = _stopped_engines(gu, engine, "peaky2")[5]
    for n in (1, 2, 2):  # (the second pass of two layers starts from the pad rows the first one left)
        eng.debug_encode(ids, lens, n)
        for i in ((11, 13, 14, 15, 17) if form["x8"] else (19, 13, 14)):
            x = eng.debug_read(i, pad_rows=True)
            assert x.shape[0] == 192
            v = gsk.e4m3_decode(x) if x.dtype == np.uint8 else x.astype(np.float64)
            assert np.isfinite(v).all(), (n, i)
        gu.record("gemm_stage_parity_pad", engine=engine, case="s64", layer=n, row_class="pad", rows=192, finite=True)


# ---- a workgroup walks a second tile ------------------------------------------------------------------------------------------------------------------------------------

WALK_B = 88
WALK_LENS = (256, 200, 130, 256, 40, 256, 177, 256)       # cycled over the 88 sequences: [CLS]-form tiles and tile_both tiles side by side
WALK_SEQS = (0, 44, 84, 85, 86, 87)                        # row tiles (= sequences at 256 keys) checked in full: the first, a middle one, the last four


def test_a_workgroup_walks_a_second_tile(gu):
    """`precise`, 88 x 256 = 22 528 tokens: 264 tiles at N = 768 against one workgroup per CU, so a workgroup computes a second tile in the residual GEMMs too
    (in the QKV projection and FFN-1, 792 and 1 056 tiles, up to a fifth) — the next tile's statistics and b' arrive by the in-loop prefetch, the next residual
    tile is parked during the epilogue.  Layer 2.  The reference covers every column of all rows of the row tiles WALK_SEQS and of the special rows of every
    sequence; which row tiles are computed second follows from launch_pp and raster_pp (gsk.later_row_tiles), and the subset has to contain them."""
    t0 = time.time()
    num_cu = 256  # the MI355X's; the engines are created with MEMVUL_NUM_CU set to it (mv_create refuses a value above the device's own count), so the grids are these
    M = WALK_B * 256
    second = gsk.later_row_tiles(M, gsk.H, num_cu)
    assert M // 256 * 3 > num_cu and second, (num_cu, second)            # a second tile exists at N = 768
    assert second <= set(WALK_SEQS), (sorted(second), WALK_SEQS)         # ... and every row tile computed second there is checked in full
    for N in (3 * gsk.H, gsk.INTER):                                     # the wider launches: every row tile has later tiles
        assert set(WALK_SEQS) <= gsk.later_row_tiles(M, N, num_cu), N
    dims, w = gu.weights_for(L2, MODELS["peaky2"])
    ids, lens = sk.boundary_ids(256, [WALK_LENS[i % len(WALK_LENS)] for i in range(WALK_B)], dims.vocab_size, seed=11)
    form = gsk.pass_form("precise", 256, lens)
    engs = _stopped_engines(gu, "precise", "peaky2", env_extra=(("MEMVUL_NUM_CU", str(num_cu)),), max_tokens=M, max_batch=WALK_B)
    seqs = np.array(WALK_SEQS)
    full, special = layer_states(engs, form, ids, lens, 2, subsets=((seqs, None), (None, gsk.special_rows(lens))))
    assert np.array_equal(full[1]["tile_both"], form["tile_both"])
    lw = gsk.layer_weights(w, 1)
    rep_full, _ = gsk.check_layer(gsk.layer_records(full, form), lw, gsk.sub_form(form, seqs), lens[seqs])
    rep_sp, _ = gsk.check_layer(gsk.layer_records(special, form), lw, form, np.full(WALK_B, 2))  # (two-token sequences: both rows special)
    _record(gu, rep_full, engine="precise", model="peaky2", case="walk_88x256_tiles", layer=2)
    _record(gu, rep_sp, engine="precise", model="peaky2", case="walk_88x256_special_rows", layer=2)
    assert engs[5].x8_saturation() == 0
    gu.record("gemm_stage_parity_case", engine="precise", model="peaky2", case="walk_88x256", seconds=time.time() - t0, worst=max(rep_full.worst(), rep_sp.worst()))
    bad = [r for r in rep_full.rows + rep_sp.rows if r["max_ratio"] > 1.0]
    assert not bad, bad
