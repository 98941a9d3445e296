"""The bounds of tests/test_stage_parity_gpu.py without a GPU: a numpy emulation of attention_v2_kernel's arithmetic (tests/stage_kit.py emulate_attention: fp32
scores, per-chunk online softmax, P to fp16 — hi + lo on the two-plane path —, fp32 P V, fp16 store) on the boundary batches with random fp16 operands at three
score scales stays inside the bound everywhere, and four faults the GPU test is there to catch each leave it on at least one boundary row:
  unmasked_key    key `len` left unmasked (thr off by one)
  no_rescale      the chunk rescale exp2(m_old - m_new) of O skipped
  neighbour_rows  the context of one work item written to its neighbour's rows (the O tile is flushed during the NEXT unit)
  v_swap          tokens 1 and len - 1 exchanged in V only (the special-row order applied to one operand and not to the others)
The reference and the bound are built by the same functions the GPU test feeds the engine's taps to."""
import numpy as np
import pytest

import stage_kit as sk

SCORE_STDS = (0.5, 2.0, 6.0)  # diffuse .. one or two keys hold the row (the peaked 2-layer model of the GPU test has 1.5 - 3)
PATHS = (("one_plane", False), ("two_plane", True))


def _applies(mutation, batch, planes2):
    """The batches a fault can show in: the rescale needs a second chunk; the exchange a row of three tokens or more; an unmasked key `len` a row shorter than
    the padded length (every batch has one); a neighbour every batch."""
    Sp, _, lens = batch
    if mutation == "no_rescale":
        return sk.chunk_keys(Sp, planes2) < Sp
    if mutation == "v_swap":
        return max(lens) >= 3
    return True


@pytest.mark.parametrize("path,planes2", PATHS)
@pytest.mark.parametrize("batch", sk.BOUNDARY_BATCHES, ids=sk.batch_id)
def test_the_emulation_stays_inside_the_bound(batch, path, planes2):
    Sp, _, lens = batch
    worst = {}
    for i, std in enumerate(SCORE_STDS):
        r = sk.emulation_ratio(Sp, lens, std, seed=100 * Sp + i, planes2=planes2)
        worst[std] = float(r.max())
    print(f"{path} {sk.batch_id(batch)}: max |emulation - float64| / bound by score scale {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert min(worst.values()) > 0.05, worst  # (the bound is not vacuous: the emulation's own roundings fill a visible part of it)


@pytest.mark.parametrize("path,planes2", PATHS)
@pytest.mark.parametrize("mutation", sk.MUTATIONS)
@pytest.mark.parametrize("batch", sk.BOUNDARY_BATCHES, ids=sk.batch_id)
def test_each_fault_leaves_the_bound(batch, mutation, path, planes2):
    Sp, _, lens = batch
    worst = {}
    for i, std in enumerate(SCORE_STDS):
        r = sk.emulation_ratio(Sp, lens, std, seed=100 * Sp + i, planes2=planes2, mutation=mutation)
        rows = r.max(axis=(1, 3))  # [B, S]: per query row, over heads and dims
        worst[std] = (float(r.max()), int((rows > 1.0).sum()))
    print(f"{path} {sk.batch_id(batch)} {mutation}: (max ratio, rows over the bound) by score scale {worst}")
    if _applies(mutation, batch, planes2):
        assert all(n >= 1 for _, n in worst.values()), worst
    else:  # nothing for the fault to touch in this batch: the emulation is the unmutated one
        assert all(m <= 1.0 for m, _ in worst.values()), worst


def test_the_faults_apply_where_the_kernel_has_the_structure():
    """Every fault is exercised on both paths, the rescale on every chunked geometry the engine launches (encoder_pass.h launch_attention)."""
    for _, planes2 in PATHS:
        for mutation in sk.MUTATIONS:
            assert any(_applies(mutation, b, planes2) for b in sk.BOUNDARY_BATCHES), (mutation, planes2)
    assert {b[0] for b in sk.BOUNDARY_BATCHES if _applies("no_rescale", b, False)} == {384, 512}
    assert {b[0] for b in sk.BOUNDARY_BATCHES if _applies("no_rescale", b, True)} == {192, 256, 384, 512}


def test_attention_terms_agree_with_the_plain_float64_attention():
    """attention_terms64 (row by row, real rows only) against attention64 (the whole batch at once), and its bound terms against their definitions."""
    lens = np.array([1, 2, 3, 40, 64])
    hi, _ = sk.random_operands(len(lens), 2, 64, lens, 2.0, 5, False)
    q, k, v = (t.astype(np.float64) for t in hi)
    t = sk.attention_terms64(q, k, v, lens)
    m = sk.row_mask(lens, q.shape)
    assert np.abs(t["ref"] - sk.attention64(q, k, v, lens, round_p=False))[m].max() < 1e-12
    assert (t["pav"] + 1e-15 >= np.abs(t["ref"]))[m].all() and (t["sp"] <= t["pav"] + 1e-15)[m].all()
    assert np.allclose(t["sp"][0, :, 0], np.abs(v[0, :, 0])) and np.allclose(t["pav"][0, :, 0], np.abs(v[0, :, 0]))  # one token: p_0 = 1, key 1 is masked
    assert np.allclose(t["sp"][1, :, :2], t["pav"][1, :, :2])                                                       # two tokens: both are special
    assert np.allclose(t["vmax"][3, :, 0, 0], np.abs(v[3, :, :40]).max(axis=(1, 2)))
