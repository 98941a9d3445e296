"""The attention bound of tests/f32_stage_kit.py and its teeth, without a GPU.

fsk.emulate_attention_f32 is attention_f32_kernel (memvul_amd/csrc/ref_f32.h) in numpy: fp32, FMA-exact, in the kernel's own order — the 64-dim contraction two k
per issue as (d, d + 32), chunks of 32 keys, per half-wave maxima and sums combined across the halves, the online rescale of l, pass 2 normalised before the P V
chain over the keys in the order the MFMA contracts them.  Not the device expf, not the MFMA's internal rounding: that is what the factor 2 in C_S is for.

On fsk.CS_TABLE (padded lengths 64 - 512, lens 1, 2, 31, 32, 33, 63, 64, 65, 97, 128, 225, 256, 385, 512, score standard deviations 1, 4, 10, 20):
  * the chain constant the emulation shows, max |ctx - ctx64| / (pav x u x smag), is the one C_S states: 2 x it lies in [0.9, 1.0] x C_S;
  * the unmutated emulation needs at most 0.5 of the bound in every case;
  * every fault of fsk.MUTATIONS reads a share > 1 on EVERY sequence of the table where it can act; the sequences where it cannot are fsk.can_act's, asserted
    here as a list (EXEMPT), not skipped.
Shares by which the faults leave the bound (printed with -s), the weakest per fault over the table: p_fp16 3.5 (len 2, std 20: a softmax that is nearly one-hot);
from len 31 on it reads 32 - 108 at std 1, 38 - 48 at std 4, 17 - 23 at std 10 and 7.5 - 13 at std 20.  Every other fault 1e4 - 1e9 (half_wave_max at len 2: NaN — the
half without a real key computes -inf - -inf).

Then the stop of an MV_F32 pass as the host source states it (encoder_pass.h encode_f32_dev, engine.hip mv_debug_read): what it accepts and what it refuses."""
import re

import numpy as np
import pytest

import f32_stage_kit as fsk
import stage_kit as sk

_f64 = np.float64
_cache = {}


def _shares(i, mutation=None):
    """Per sequence of table case i: (max share of the bound, max chain constant shown) over its real rows, heads and dims."""
    Sp, lens, std = fsk.CS_TABLE[i]
    if i not in _cache:
        if len(_cache) >= 1:  # (the mutation tests walk the table case by case: one set of operands and scores alive)
            _cache.clear()
        q, k, v = fsk.table_operands(Sp, lens, std)
        _cache[i] = (q, k, v, fsk.emulate_scores(q, k), tuple(x.astype(_f64) for x in (q, k, v)))
    q, k, v, s, f = _cache[i]
    out = fsk.emulate_attention_f32(q, k, v, lens, mutation, scores=s)
    if mutation != "half_wave_max":  # (the fault whose output may be NaN)
        assert np.isfinite(out).all()
    share, chain = fsk.attention_share(out.astype(_f64), *f, lens)
    return [(float(share[b].max()), float(chain[b].max())) for b in range(len(lens))]


@pytest.fixture(scope="module")
def clean():
    return [_shares(i) for i in range(len(fsk.CS_TABLE))]


def test_the_table_holds_every_chunk_edge():
    lens = {n for _, ls, _ in fsk.CS_TABLE for n in ls}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 97, 225, 385, 512} <= lens
    assert {Sp for Sp, _, _ in fsk.CS_TABLE} == {64, 128, 256, 512} and {std for _, _, std in fsk.CS_TABLE} == {1.0, 4.0, 10.0, 20.0}


def test_the_chain_constant_is_the_measured_one(clean):
    by_std = {}
    for (Sp, lens, std), rows in zip(fsk.CS_TABLE, clean):
        c = max(ch for _, ch in rows)
        by_std.setdefault(std, []).append(c)
        print(f"Sp {Sp} std {std:g}: chain constant {c:.3f}, share of the bound {max(sh for sh, _ in rows):.3f}")
    for std, cs in sorted(by_std.items()):
        print(f"std {std:g}: {min(cs):.2f} - {max(cs):.2f}")
    measured = max(max(cs) for cs in by_std.values())
    assert 0.9 * fsk.C_S <= 2.0 * measured <= fsk.C_S, (measured, fsk.C_S)


def test_unmutated_emulation_stays_within_half_of_the_bound(clean):
    worst = {(Sp, n, std): sh for (Sp, lens, std), rows in zip(fsk.CS_TABLE, clean) for n, (sh, _) in zip(lens, rows)}
    assert max(worst.values()) <= 0.5, {k: v for k, v in worst.items() if v > 0.5}


def test_emulation_against_plain_float32_attention():
    """The emulation is attention: against softmax(q k^T) v formed in fp32 by matrix products it differs by roundings only (2e-5 of max |v|), at a length on
    no chunk edge, and the rows past len are computed like any other."""
    Sp, lens = 128, (77, 128)
    q, k, v = fsk.table_operands(Sp, lens, 4.0)
    out = fsk.emulate_attention_f32(q, k, v, lens)
    ref = sk.attention64(*(x.astype(_f64) for x in (q, k, v)), lens, round_p=False)
    assert np.isfinite(out).all()
    assert float(np.abs(out - ref).max()) <= 2e-5 * float(np.abs(v).max())


# (mutation, len, Sp) where the fault cannot act: what fsk.can_act answers over the table, spelled out
EXEMPT = {
    "mask_len_plus_1": {(64, 64), (128, 128), (256, 256), (512, 512)},      # there is no key `len`
    "mask_len_minus_1": {(1, 64)},                                         # the kernel clamps len to 1
    "half_wave_max": {(1, 64)},
    "no_rescale": {(1, 64), (2, 64), (31, 64), (32, 64)},                  # a single chunk
    "key_map": {(1, 64), (2, 64)},                                         # keys 0 - 7 sit in registers 0 - 3 under either map
    "d_half": set(),
    "p_fp16": {(1, 64)},                                                   # p = 1 is an fp16 number
}


def test_exemptions_are_the_listed_ones():
    assert set(EXEMPT) == set(fsk.MUTATIONS)
    seqs = {(n, Sp) for Sp, lens, _ in fsk.CS_TABLE for n in lens}
    for mut in fsk.MUTATIONS:
        assert {x for x in seqs if not fsk.can_act(mut, *x)} == EXEMPT[mut], mut


@pytest.mark.parametrize("mutation", fsk.MUTATIONS)
def test_mutation_leaves_the_bound_wherever_it_can_act(mutation):
    factors = {}
    for i, (Sp, lens, std) in enumerate(fsk.CS_TABLE):
        for n, (sh, _) in zip(lens, _shares(i, mutation)):
            if (n, Sp) not in EXEMPT[mutation]:
                factors[(Sp, n, std)] = sh
    weakest = min(factors, key=factors.get)
    print(f"{mutation}: weakest x{factors[weakest]:.3g} at (Sp, len, std) = {weakest}; {len(factors)} sequences")
    assert all(f > 1.0 for f in factors.values()), {k: f for k, f in factors.items() if not f > 1.0}


# ---- the stop of an MV_F32 pass, as the host source states it ---------------------------------------------------------------------------------------------------------

def _f32_pass_body():
    src = sk.host_source()
    m = re.search(r"int encode_f32_dev\(.*?\n}\n", src, flags=re.S)
    assert m
    return src, m.group(0)


def test_stop_ends_the_reference_pass_after_each_launch_group():
    src, body = _f32_pass_body()
    # encode_dev hands the stop over instead of refusing it, and only mv_debug_encode's passes (full) carry one
    assert "const int stop = full ? h->dbg_stop : 0;" in src
    assert re.search(r"if \(h->f32\) return encode_f32_dev\([^;]*pitch, stop\);", src)
    assert "the stop inside a layer exists on the persistent path of MV_F16 / MV_F16X8 only" not in src
    # the launches of a layer in order, each stop right behind its group, in the LAST layer only
    assert "const int ls = l == n_layers - 1 ? stop : 0;" in body
    marks = ["KC_GEMM_QKV", "if (ls == 1) return MV_OK;", "attention_f32_kernel", "if (ls == 2) return MV_OK;", "KC_GEMM_OUT", "if (ls == 3) return MV_OK;",
             "run_ln(w.ln1g, w.ln1b)", "KC_GEMM_FFN1", "if (ls == 4) return MV_OK;", "KC_GEMM_FFN2", "if (ls == 5) return MV_OK;", "run_ln(w.ln2g, w.ln2b)", "pool_head("]
    pos = [body.find(x) for x in marks]
    assert all(p >= 0 for p in pos) and pos == sorted(pos), list(zip(marks, pos))
    # no layers: the embedding as it is, ahead of the layer loop
    assert 0 <= body.find("if (stop && n_layers == 0) return MV_OK;") < body.find("for (int l = 0; l < n_layers; ++l)")
    # the switch: development build only, 1 .. 5
    dev = src[src.index("#ifdef MEMVUL_DEV_SWITCHES"):]
    assert 'env_int("MEMVUL_DEBUG_STOP", 1, 5, &h->dbg_stop)' in dev[:dev.index("#endif")]
    assert src.count("MEMVUL_DEBUG_STOP\"") == 1


def test_taps_of_the_reference_form_in_the_host_source():
    src, _ = _f32_pass_body()
    read = src[src.index("int mv_debug_read("):]
    read = read[:read.index("catch (...)")]
    for buf, plane, width in ((35, "qkv32", "3 * MV_HIDDEN"), (36, "ctx32", "MV_HIDDEN"), (37, "h32", "MV_INTER")):
        assert f"case {buf}: src = wk.{plane}; avail = T * {width} * 4; break;" in read
    # ahead of the development-only taps: the product library has them too
    assert read.index("case 37:") < read.index("#if defined(MEMVUL_DEV_SWITCHES)")
    # another dtype never allocates the planes (workspace.h), so the null-plane answer is theirs
    assert 'if (!src) return fail(h, MV_ERR_STATE, "mv_debug_read: this buffer does not exist in this compute dtype");' in read
    assert re.search(r"group == MV_F32\) \{[^}]*A\(&wk\.qkv32[^}]*A\(&wk\.ctx32[^}]*A\(&wk\.h32[^}]*\}", src)
    assert len(re.findall(r"A\(&wk\.(?:qkv32|ctx32|h32),", src)) == 3
    # 1 - 9 still refuse on MV_F32, in words the GPU test matches on
    assert re.search(r"if \(h->f32 && buffer >= 1 && buffer <= 9\)\s*return fail\(h, MV_ERR_INVALID, \"[^\"]*fp16[^\"]*35 - 37", read)


def test_binding_shapes_of_the_reference_taps():
    import inspect

    from memvul_amd import binding

    text = inspect.getsource(binding.Engine.debug_read)
    assert "35: ((B, Sp, 3 * 768), np.float32), 36: ((B, Sp, 768), np.float32), 37: ((B, Sp, 3072), np.float32)" in text
    assert not {35, 36, 37} & set(binding.Engine._TOKEN_AXIS)  # token order as they lie: no special-row swap
