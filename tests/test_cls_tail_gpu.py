"""Every launch of the pruned last layer's [CLS] tail on the engine's own operands (tests/cls_tail_kit.py): cls_gather_kernel, the Q projection, attention_cls_kernel,
output projection + residual, LayerNorm, FFN-1, FFN-2 + residual, LayerNorm, pooler, header — element by element, every real row and every column.

The tail is what every product forward runs (MEMVUL_CLS_PRUNE defaults to on) and what mv_debug_encode never shows (its last layer is un-pruned).  The development
build's MEMVUL_DEBUG_TAIL=1 copies what each launch of the tail wrote into a tap arena (mv_debug_read 22 - 34) during an ORDINARY encode; the taps of the tail's
inputs (the stream, its low parts and vstats; K, V^T, their lo planes, vlo_sp) still hold them after that call.  Each launch's float64 model is formed from the
tapped operands of THAT launch; the bounds are derived (the kit's docstring) and fixed on a numpy emulation in tests/test_cls_tail_cpu.py.  Asserted: every
tapped stage finite and within its bound; c16 exact given c32; the tapped u equal, bit for bit, to encode() of the library without the taps.  Recorded per
launch, engine and model: the worst and the rms share of the bound used (profiles/cls_tail_parity.md).

The last test settles what the pruned layer reads at padded lengths <= 128 in the default form of MV_F16X8: V of every key as ONE fp16 plane (no lo plane, no
vlo_sp), under a [SEP] sink — the logits against the float64 oracle, pruned and with MEMVUL_CLS_PRUNE=0."""
import time
import warnings

import numpy as np
import pytest

import cls_tail_kit as kit
import stage_kit as sk

pytestmark = pytest.mark.gpu

L2 = dict(layers=2, vocab_size=2048)
LOGIT_TOL = 1e-3  # the project's contract on the logits


class _Sink(dict):
    """The `sink` argument of synth.make_weights in a form gpu_util's caches can key on."""

    def __hash__(self):
        return hash(tuple(sorted(self.items())))


def sink_kw(layers):
    return dict(kit.SINK_KW, seed=kit.SINK_SEED, sink=_Sink(token="sep", rows="cls", gains=tuple(kit.SINK_GAINS[:layers])))


MODELS = {"peaky2": dict(qk_scale=4.0), "outliers2": dict(qk_scale=4.0, ln_outliers=True), "sep_sink2": sink_kw(2)}
# name: (kit kind, compute dtype, engine_for keywords, weight keywords on top of the model's, the library the bit-for-bit comparison runs on)
ENGINES = {
    "precise": ("precise", "precise", {}, {}, "product"),
    "safe": ("safe", "safe", {}, {}, "product"),
    "f16_tile512": ("f16", "f16", dict(gemm_tile=512), {}, "dev"),   # big path: the xlo gather (MEMVUL_GEMM_TILE is a development switch: no product library takes this path at this size)
    "f16": ("f16", "f16", {}, {}, "product"),                        # small path; the tail's GEMMs take the 64^2 ring
    "f16_tile128": ("f16", "f16", dict(gemm_tile=128), {}, "dev"),   # small path; the tail's GEMMs take gemm128
    "precise_no_header": ("precise", "precise", dict(proj_dim=768), dict(use_header=False), "product"),  # P = 768: the pooler writes u itself
}
# name: (padded length, lengths): B = 1 (three idle waves of a 4-wave block, 31 clamped rows), B = 5 (B % 4 != 0), B = 33 (a second 32-row block with one real
# row); one to eight 64-key PV blocks (512 fills ps[4][512]); lengths on the mask's edges, below 16, Sp - 1 and Sp.  B x Sp <= 4096
PASSES = {
    "b1_s64": (64, (63,)),
    "b5_s64": (64, (2, 3, 7, 9, 64)),
    "b33_s64": (64, tuple((2, 3, 7, 9, 63, 64)[i % 6] for i in range(33))),
    "b5_s128": (128, (65, 127, 128, 9, 64)),
    "b5_s192": (192, (191, 192, 65, 7, 63)),
    "b5_s256": (256, (255, 256, 64, 3, 65)),
    "b5_s384": (384, (383, 384, 65, 9, 2)),
    "b5_s512": (512, (511, 512, 63, 7, 65)),
}
ENG_KW = dict(max_tokens=4096, max_batch=40, max_anchors=8)
CASES = [(e, m) for e in ENGINES for m in MODELS if e != "precise_no_header" or m == "peaky2"]


_owned = {}  # the engines of the configuration being tested (the tapped one and the one without taps): this module's own, so that it evicts nobody else's from gpu_util's cache


@pytest.fixture(scope="module")
def gu():
    import gpu_util

    yield gpu_util
    _close_owned()


def _close_owned():
    for e in _owned.values():
        e.close()
    _owned.clear()


def _make(gu, dims_kw, w_kw, compute, env, dev, **kw):
    """One engine with `env` set while mv_create reads its switches (what gpu_util.engine_for does, without its cache)."""
    import os

    from memvul_amd import binding

    dims, w = gu.weights_for(dims_kw, w_kw)
    switches = ("MEMVUL_CLS_PRUNE", "MEMVUL_STREAMS", "MEMVUL_QKV_ASIDE", "MEMVUL_CLS_ASIDE", "MEMVUL_CLS_ASIDE_MIN_LEN", "MEMVUL_FORM") + binding.DEV_SWITCHES
    old = {k: os.environ.pop(k, None) for k in switches}
    os.environ.update(env)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the default form warns once about a sink it sees)
            e = binding.Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_pos=dims.max_pos, dev=dev, **kw)
            e.load_state_dict(w, compute)
    finally:
        for k in switches:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return e


def _engine(gu, engine, model, taps):
    _, compute, kw, wkw, plain = ENGINES[engine]
    key = (engine, model, taps)
    if key not in _owned:
        if any(k[:2] != (engine, model) for k in _owned):
            _close_owned()
        kw = dict(ENG_KW, **kw)
        tile = kw.pop("gemm_tile", 0)
        env = {"MEMVUL_GEMM_TILE": str(tile)} if tile else {}
        if taps:
            env["MEMVUL_DEBUG_TAIL"] = "1"
        _owned[key] = _make(gu, L2, dict(MODELS[model], **wkw), compute, env, dev=taps or plain == "dev", **kw)
    return _owned[key]


def _quiet(f, *a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a)


@pytest.mark.parametrize("engine,model", CASES)
def test_each_launch_of_the_cls_tail_on_its_own_operands(gu, engine, model):
    kind, _, kw, wkw, plain = ENGINES[engine]
    dims, w = gu.weights_for(L2, dict(MODELS[model], **wkw))
    tw = kit.tail_weights(w, dims.layers, fp16_ops=(kind == "f16"))
    big = kind != "f16" or kw.get("gemm_tile") == 512
    P = kw.get("proj_dim", 512)
    t0 = time.time()
    eng = _engine(gu, engine, model, taps=True)
    inputs, tapped_u, worst = {}, {}, {}
    bad = []
    for name, (Sp, lens) in PASSES.items():
        ids, lens = sk.boundary_ids(Sp, lens, dims.vocab_size, seed=13)
        inputs[name] = (ids, lens)
        before = eng.debug_read(34) if name != next(iter(PASSES)) else None
        u = _quiet(eng.tail_encode, ids, lens)
        info = eng.debug_read(34)
        assert tuple(info[1:]) == (len(lens), Sp), info                      # the batch ran as one pass of B rows at this padded length ...
        assert before is None or info[0] == before[0] + 1, (before, info)   # ... and as one pruned pass
        taps = kit.read_tail_taps(eng, kind, big, lens)
        for k, v in taps.items():
            if k not in ("k", "v", "sp_keys", "vlo_sp", "hi", "lo", "vst", "x32", "x16"):
                assert np.isfinite(v).all(), (name, k)
        assert np.array_equal(taps["u"].astype(np.float32), u), name        # tap 33 is what the call returned
        tapped_u[name] = u
        shares = kit.check_tail(taps, tw, kind, big, lens, P)
        for launch, r in shares.items():
            mx, rms = kit.stats(r)
            print(f"{engine} {model} {name} {launch}: worst {mx:.3f} rms {rms:.3f}")
            w0 = worst.get(launch, (0.0, 0.0, 0))
            worst[launch] = (max(w0[0], mx), np.sqrt((w0[1] ** 2 * w0[2] + rms ** 2 * r.size) / (w0[2] + r.size)), w0[2] + r.size)
            if not mx <= 1.0:
                bad.append((name, launch, mx))
    if kind != "f16":
        assert eng.x8_saturation() == 0
    for launch, (mx, rms, _) in worst.items():
        gu.record("cls_tail_parity", engine=engine, model=model, launch=launch, max_share=mx, rms_share=float(rms))
    # the taps change nothing: the same inputs through the library without them, bit for bit
    ref = _engine(gu, engine, model, taps=False)
    for name, (ids, lens) in inputs.items():
        assert np.array_equal(_quiet(ref.encode, ids, lens), tapped_u[name]), (name, plain)
    gu.record("cls_tail_parity_case", engine=engine, model=model, seconds=time.time() - t0, worst=max(v[0] for v in worst.values()))
    assert not bad, bad


# ---- the pruned layer at padded lengths <= 128 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layers", [2, 4])
def test_pruned_last_layer_holds_the_contract_at_64_and_128_keys_under_a_sep_sink(gu, layers):
    """Default form of MV_F16X8, padded lengths 64 and 128: such a pass is a two-plane pass, so attention_cls_kernel gets no vlo_sp, and the pruned layer's K / V
    launch writes no lo planes outside the safe form — the single-query attention reads V of [CLS] and [SEP] as one fp16 plane, where every earlier layer of the
    pass carries hi + lo.  With 80 % of the [CLS] row's mass on [SEP] that is the fp16 storage error of ONE key reaching the pooler un-averaged: the logits
    against the float64 oracle, pruned (asserted: the 1e-3 contract) and with MEMVUL_CLS_PRUNE=0 (the full last layer through the two-plane attention; recorded)."""
    from memvul_amd import synth
    from oracle import memvul_oracle as orc

    dk = dict(layers=layers, vocab_size=2048)
    wkw = sink_kw(layers)
    dims, w = gu.weights_for(dk, wkw)
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items() if np.asarray(v).ndim}
    _close_owned()
    engs = {"pruned": _make(gu, dk, wkw, "precise", {}, False, **ENG_KW), "unpruned": _make(gu, dk, wkw, "precise", {"MEMVUL_CLS_PRUNE": "0"}, False, **ENG_KW)}
    _owned.update({("short", layers, k): e for k, e in engs.items()})
    for Sp in (64, 128):
        ids, lens = sk.boundary_ids(Sp, (Sp, Sp - 1, Sp // 2 + 1, 17, 40, Sp, 9, Sp - 7), dims.vocab_size, seed=21)
        aids, alens = sk.boundary_ids(Sp, (Sp, Sp - 3, 33, 20), dims.vocab_size, seed=22)
        assert synth.sink_token_id("sep") == ids[0, lens[0] - 1]
        f = lambda i, n: orc.instance_forward(w64, i.astype(np.int64), np.arange(i.shape[1])[None, :] < n[:, None], dtype=np.float64)  # noqa: E731
        want = orc.match(f(ids, lens), f(aids, alens), w64["_projector.weight"])[0]
        err = {}
        for name, eng in engs.items():
            eng.anchor_reset()
            _quiet(eng.anchor_append, aids, alens)
            got = _quiet(eng.forward, ids, lens)["logits"]
            eng.anchor_reset()
            assert np.isfinite(got).all()
            err[name] = float(np.abs(got - want).max())
        print(f"sep sink, {layers} layers, {Sp} keys: logits error pruned {err['pruned']:.3e}, MEMVUL_CLS_PRUNE=0 {err['unpruned']:.3e} (|logit| up to {np.abs(want).max():.2f})")
        gu.record("cls_tail_short_pass", layers=layers, Sp=Sp, pruned=err["pruned"], unpruned=err["unpruned"], logit_scale=float(np.abs(want).max()))
        assert err["pruned"] <= LOGIT_TOL, err
