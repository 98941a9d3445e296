"""The concentration monitor's float64 reference (oracle/concentration.py) and its committed fixture (tests/golden/monitor_refs.npz, scripts/make_monitor_refs.py),
the parts that need no GPU: the fixture is the oracle's output, it still meets the conditions the GPU tests rely on, and the per-sequence rule restated in numpy
agrees with the numbers the engine's sources state."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_monitor_refs as mk  # noqa: E402
from oracle import concentration as conc  # noqa: E402


@pytest.fixture(scope="module")
def refs(golden_dir):
    return np.load(os.path.join(golden_dir, "monitor_refs.npz"))


def test_fixture_holds_every_case_and_nothing_else(refs):
    want = {"delta_abs"} | {m + "_gains" for m in mk.MODELS} | {"%s_%d_%s" % (m, W, f) for m in mk.MODELS for W in mk.WIDTHS for f in ("exact",) + mk.FORMS}
    want |= {"batch_%d_%d_exact" % bs for bs in mk.BATCHES} | {"guarded_%s_exact" % c for c in mk.GUARDED_CASES}
    assert set(refs.files) == want
    for k in refs.files:
        assert refs[k].dtype == (np.float32 if k.endswith("_gains") else np.float64), k
    for m in mk.MODELS:
        for W in mk.WIDTHS:
            assert refs["%s_%d_exact" % (m, W)].shape == (3, 8, 12)
    for B, S in mk.BATCHES:
        assert refs["batch_%d_%d_exact" % (B, S)].shape == (3, B, 12)
    for c in mk.GUARDED_CASES:
        assert refs["guarded_%s_exact" % c].shape == (11, 28, 12)


def test_fixture_inputs_cover_the_lengths_and_the_sink_positions():
    """What scripts/make_monitor_refs.py promises about the sequences, on the inputs the GPU tests rebuild."""
    from memvul_amd import synth

    for W in mk.WIDTHS:
        prev = ([0] + list(mk.WIDTHS))[mk.WIDTHS.index(W)]
        met, in_chunk = set(), set()
        for k, m in enumerate(mk.MODELS):
            ids, lens, pos, names = mk.case_inputs(m, W)
            assert ids.shape == (8, W) and {W, W - 1, 15, 16, 17} <= set(lens.tolist()) and (not prev or prev + 1 in lens)
            assert int(lens.max()) == W and int(lens.min()) == 15
            for b, n in enumerate(lens):
                n = int(n)
                assert ids[b, 0] == synth.CLS_ID and ids[b, n - 1] == synth.SEP_ID and not ids[b, n:].any() and ids[b, 1:n - 1].min() >= 1000
                where = np.flatnonzero(ids[b] == synth.MID_ID)
                assert where.tolist() == ([] if pos[b] < 0 else [pos[b]]) and (pos[b] < 0 or 1 <= pos[b] <= n - 2), (m, W, b)
                met.add((names[b], n))
                if names[b].startswith("chunk") and mk.MODELS[m][0] == "mid":
                    in_chunk.add((names[b], pos[b] // 128))
        # over the models, the sink on the first and on the last ordinary token meets the full width, the width minus one and the 16-token row
        for kind in ("first", "last"):
            assert {(kind, W), (kind, W - 1), (kind, 16)} & met, (W, kind, sorted(met))
        if W > 256:  # on the models with an ordinary-token sink: a row with the sink inside every 128-key chunk, those after the first included
            for c in range(W // 128):
                assert ("chunk%d" % c, c) in in_chunk, (W, c, sorted(in_chunk))
    for B, S in mk.BATCHES:
        ids, lens, pos = mk.batch_inputs(B, S)
        assert ids.shape == (B, S) and lens[2] == 15 and lens[3] == 16 and (pos[0::2] >= 1).all() and (pos[1::2] == -1).all()


@pytest.mark.parametrize("model,W", [("mid_cls_50", 128), ("sep_cls_80", 64)])
def test_fixture_is_the_oracles_output(refs, model, W):
    """One small case regenerated through oracle/concentration.py from the stored gains: the exact array to 1e-12 (float64 sums in another order), and the
    shipped-default model array — the fixture is pinned to the oracle, not to a copy of it."""
    ids, lens, _, _ = mk.case_inputs(model, W)
    w = mk.weights(model, refs[model + "_gains"])
    ex = conc.cls_collision(w, ids, lens)
    assert ex.shape == (3, 8, 12) and np.abs(ex - refs["%s_%d_exact" % (model, W)]).max() <= 1e-12
    if model == "mid_cls_50":
        cfg, kw = mk.model_cfg("shipped")
        assert np.abs(conc.cls_collision(w, ids, lens, cfg, **kw) - refs["%s_%d_shipped" % (model, W)]).max() <= 1e-12


def test_the_oracle_excludes_the_first_and_the_last_token_only():
    """cls_collision on a hand-made probability row: every key but [CLS] and [SEP] is counted, in the sequence's own order, padding never."""
    from oracle import precision_model as pm

    calls = []

    def fake_forward(w, ids, mask, cfg, **kw):
        B, S = ids.shape
        e = np.zeros((B, 12, S, S))
        e[:, :, 0, :] = np.array([4.0, 3.0, 2.0, 1.0, 6.0, 100.0])[None, None, :] * mask[:, None, :]
        for l in range(3):
            calls.append(pm.FORMATS[cfg["p"][l]](e) is e)
        return "out"

    w = {pm.PFX + "encoder.layer.%d.attention.self.query.weight" % l: None for l in range(3)}
    ids, lens = np.ones((2, 6), np.int64), np.array([5, 4])
    coll, out = conc.cls_collision(w, ids, lens, forward=fake_forward, with_output=True)
    assert out == "out" and calls == [True] * 3 and coll.shape == (3, 2, 12)
    assert np.allclose(coll[:, 0], (3.0 ** 2 + 2.0 ** 2 + 1.0 ** 2) / 16.0 ** 2, rtol=0, atol=1e-15)  # len 5: keys 1, 2, 3 of 4 + 3 + 2 + 1 + 6
    assert np.allclose(coll[:, 1], (3.0 ** 2 + 2.0 ** 2) / 10.0 ** 2, rtol=0, atol=1e-15)            # len 4: keys 1, 2 of 4 + 3 + 2 + 1


def test_fixture_meets_the_conditions_the_gpu_tests_rely_on(refs):
    """scripts/make_monitor_refs.py check() on the stored arrays: delta as stored, at most 5 % of a case's items inside the band, every graded case with a fifth
    of its items on either side, a quarter of the graded rows with a verdict no band item can change, both verdicts at every width."""
    delta_abs = mk.check(refs, verbose=False)
    assert delta_abs == float(refs["delta_abs"]) and 1e-4 < delta_abs < 1e-2, delta_abs
    # the controls: the sink sits on an excluded key, the collision mass on the ordinary keys of every row of at least 64 tokens is far below the threshold;
    # the sinks on the first and on the last ordinary token are far above it somewhere in every graded model (a monitor that dropped that key would read low)
    for m in ("sep_cls_80", "cls_all_80"):
        for W in mk.WIDTHS:
            lens = mk.case_inputs(m, W)[1]
            assert refs["%s_%d_exact" % (m, W)][:, lens >= 64].max(initial=0.0) < 0.2, (m, W)  # (0.8^2 = 0.64 if the sink key were counted)
    for m, spec in mk.MODELS.items():
        if not spec[4]:
            continue
        top = {"first": 0.0, "last": 0.0}
        for W in mk.WIDTHS:
            _, lens, _, names = mk.case_inputs(m, W)
            for b, kind in enumerate(names):
                if kind in top and lens[b] >= 64:
                    top[kind] = max(top[kind], float(refs["%s_%d_exact" % (m, W)][:, b].max()))
        assert min(top.values()) > 0.4, (m, top)


def test_the_rule_in_numpy_agrees_with_the_numbers_the_sources_state():
    """over > 0.02 x 12 x monitored layers, no items below 16 tokens: 132 items (12 layers, the last one pruned) rescore at >= 3, 12 items (2 layers) at >= 1."""
    from stage_kit import host_source

    src = host_source()
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    att = open(os.path.join(ROOT, "memvul_amd", "csrc", "attention.h")).read()
    kern = open(os.path.join(ROOT, "memvul_amd", "csrc", "attention_v2.h")).read()
    assert float(re.search(r"constexpr double kGuardShare = ([0-9.]+);", src).group(1)) == conc.GUARD_SHARE
    assert float(re.search(r"#define MV_SINK_COLLISION ([0-9.]+)f", att).group(1)) == conc.THRESHOLD
    assert re.search(r"const int items = len >= %d \? MV_HEADS \* layers : 0;" % conc.MIN_LEN, src)
    assert kern.count("if (lane == 0 && len >= %d)" % conc.MIN_LEN) == 2  # the one-chunk and the chunked path
    assert "more than 2 % of its own monitored (head, layer) items above a collision mass of" in hdr and "a sequence of fewer than 16 tokens has no items" in hdr
    gpu_doc = open(os.path.join(ROOT, "tests", "test_guarded_form_gpu.py")).read()
    assert "132 monitored per sequence; rescored at >= 3" in gpu_doc and "12 items per sequence, rescored at >= 1" in gpu_doc
    over = np.arange(0, 6)
    assert conc.items_total([256], 11)[0] == 132 and conc.rule(over, np.full(6, 256), 11).tolist() == [False, False, False, True, True, True]
    assert conc.items_total([256], 1)[0] == 12 and conc.rule(over, np.full(6, 16), 1).tolist() == [False, True, True, True, True, True]
    assert conc.items_total([15, 16], 11).tolist() == [0, 132]
    # 36 items (3 layers unpruned) and 24 (pruned): the fixture's models rescore at >= 1
    assert conc.rule([0, 1], [64, 64], 3).tolist() == [False, True] and conc.rule([0, 1], [64, 64], 2).tolist() == [False, True]
    # a sequence the monitor does not look at has no count to be flagged by
    lo, hi, v_lo, v_hi = mk.verdicts(np.full((3, 2, 12), 0.9), np.array([15, 16]), 1e-3, 2)
    assert lo.tolist() == [0, 24] and hi.tolist() == [0, 24] and v_lo.tolist() == [False, True] and v_hi.tolist() == [False, True]
