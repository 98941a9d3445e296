"""The fixed-form persistent GEMMs (memvul_amd/csrc/gemm_pp_fixed.hip, libmemvul_pp_fixed.so) against the run-time form of the same tree, bit for bit.

Two precise engines of the development build per case, one per value of MEMVUL_PP_FORM, the same seeded ids: the encode() output, every debug tap after 1 and 2
layers (scripts/pass_fingerprint.py has the tap list), and the launches per kernel class must be equal; the fixed-launch counter (Engine.pp_fixed_launches) must be
what encoder_pass.h pp_fixed_form implies — every persistent GEMM launch of a pass it holds for, none of any other pass — and 0 on the runtime engine.  No tolerance
anywhere: the contract is equality, and the reference is the run-time form in the same process.

mv_test_gemm_pp launches FFN-1 with out8_hi_only = 0 (it returns both fp8 planes), which is not the form the fixed FFN-1 kernel holds, so the hook stays on the
run-time kernel under either value of the switch; the hook case below pins that (equal bytes, counter 0)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.gpu

import gpu_util as gu  # noqa: E402
import pass_fingerprint as pf  # noqa: E402
import stage_kit as sk  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402

LAYERS = pf.DIMS["layers"]
GEMM_CLASSES = ("gemm_qkv", "gemm_attn_out", "gemm_ffn1_gelu", "gemm_ffn2", "gemm_kv_last")
CLS_MIN_LEN = 128  # the library's default (MEMVUL_CLS_ASIDE_MIN_LEN)
SWITCHES = ("MEMVUL_PP_FORM", "MEMVUL_CLS_PRUNE", "MEMVUL_CLS_ASIDE", "MEMVUL_QKV_ASIDE", "MEMVUL_CLS_ASIDE_MIN_LEN", "MEMVUL_FORM", "MEMVUL_STREAMS")


def make_engine(form, env, max_tokens):
    dims, w = gu.weights_for(pf.DIMS, pf.WEIGHTS)
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ["MEMVUL_PP_FORM"] = form
    try:
        eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_pos=dims.max_pos, dev=True, max_tokens=max_tokens, max_batch=128, max_anchors=8)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load_state_dict(w, "precise")
    return eng


class Pair:
    """The two engines of one environment: .fixed and .runtime."""

    def __init__(self, env=None, max_tokens=4096):
        self.fixed = make_engine("fixed", env or {}, max_tokens)
        self.runtime = make_engine("runtime", env or {}, max_tokens)

    def close(self):
        self.fixed.close()
        self.runtime.close()


@pytest.fixture(scope="module")
def default_pair():
    p = Pair(max_tokens=86 * 256)  # = 43 * 512: the largest passes below run as ONE pass
    yield p
    p.close()


def lengths(B, width, seed):
    """B lengths in [cls_min_len, width], not all equal: the shortest and the longest allowed are both there when B > 1."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(CLS_MIN_LEN, width + 1, size=B)
    lens[0] = width
    if B > 1:
        lens[-1] = CLS_MIN_LEN
    return tuple(int(x) for x in lens)


def run(eng, ids, lens):
    """encode() with its launches per class and its fixed launches, then every tap after 1 and 2 layers with theirs."""
    rec = {}
    eng.pp_fixed_launches(reset=True)
    eng.profile_read()
    eng.profile_enable(True)
    rec["encode"] = eng.encode(ids, lens).tobytes()
    prof = eng.profile_read()
    eng.profile_enable(False)
    rec["launches"] = {k: n for k, (_, n) in prof.items()}
    rec["encode_fixed"] = eng.pp_fixed_launches(reset=True)
    rec["taps"] = {}
    for n_layers in range(1, LAYERS + 1):
        eng.debug_encode(ids, lens, n_layers)
        for buf in sorted({b for _, b in pf.TAPS}):
            try:
                rec["taps"][(n_layers, buf)] = eng.debug_read(buf).tobytes()
            except RuntimeError:  # (a buffer this compute dtype does not have: the library says so, to both engines alike)
                rec["taps"][(n_layers, buf)] = b"-"
    rec["taps_fixed"] = eng.pp_fixed_launches(reset=True)
    return rec


def check(pair, width, lens, *, fixed_applies, prune=True, seed=0):
    ids, lens = sk.boundary_ids(width, lens, pf.DIMS["vocab_size"], seed=seed)
    a, b = run(pair.fixed, ids, lens), run(pair.runtime, ids, lens)
    assert b["encode_fixed"] == 0 and b["taps_fixed"] == 0  # the runtime engine never leaves its own kernels
    assert a["launches"] == b["launches"]
    gemm_launches = sum(a["launches"][c] for c in GEMM_CLASSES)
    per_encode = 4 * (LAYERS - 1) + 1 if prune else 4 * LAYERS  # QKV, output projection, FFN-1, FFN-2 per whole layer; the pruned last layer's K/V launch
    if fixed_applies:  # every persistent GEMM launch of the pass, and the debug passes' (unpruned: 4 per layer, 1 and then 2 layers)
        assert gemm_launches == per_encode, a["launches"]  # (one pass: the batch was not cut)
        assert a["encode_fixed"] == per_encode and a["taps_fixed"] == 4 * sum(range(1, LAYERS + 1))
    else:
        assert a["encode_fixed"] == 0 and a["taps_fixed"] == 0
    assert a["encode"] == b["encode"], "encode() differs between the two forms"
    assert sum(len(v) > 1 for v in a["taps"].values()) >= 16  # (the taps are there to compare)
    for key in a["taps"]:
        assert a["taps"][key] == b["taps"][key], "tap %d after %d layer(s) differs between the two forms" % (key[1], key[0])


# B = 1: one row tile, a grid smaller than the chip, no workgroup has a next tile; 5: Mpad > M; 86 (43 at 512): 258 output-projection / FFN-2 tiles and 1 032 FFN-1
# tiles — every kernel kind has a workgroup that walks a second tile (the prefetch of the next tile's residual and statistics)
@pytest.mark.parametrize("width,B", [(256, 1), (256, 5), (256, 86), (512, 1), (512, 43)])
def test_long_passes_take_the_fixed_form_and_keep_their_bits(default_pair, width, B):
    check(default_pair, width, lengths(B, width, seed=B), fixed_applies=True, seed=B)


def test_narrow_input_of_a_long_pass(default_pair):
    """An input narrower than its padded length (250 -> 256): the same pass, the same form."""
    check(default_pair, 250, (250, 128, 199), fixed_applies=True, seed=3)


def test_unpruned_last_layer():
    pair = Pair({"MEMVUL_CLS_PRUNE": "0"})
    try:
        check(pair, 256, lengths(5, 256, seed=11), fixed_applies=True, prune=False, seed=11)
    finally:
        pair.close()


@pytest.mark.parametrize("width,lens", [
    (256, (256, CLS_MIN_LEN - 1, 200)),  # one sequence shorter than cls_min_len: its tile runs the both-terms form, so the pass keeps the run-time kernels
    (192, (129, 150, 192, 192)),         # the whole-pass [CLS]-row form: a tile spans two sequences
    (128, (128, 100)),                   # two planes
])
def test_other_passes_fall_back(default_pair, width, lens):
    check(default_pair, width, lens, fixed_applies=False, seed=5)


def test_safe_form_falls_back(default_pair):
    for eng in (default_pair.fixed, default_pair.runtime):
        eng.set_form("safe")
    try:
        check(default_pair, 256, lengths(3, 256, seed=7), fixed_applies=False, seed=7)
    finally:
        for eng in (default_pair.fixed, default_pair.runtime):
            eng.set_form("default")


@pytest.mark.parametrize("env", [{"MEMVUL_CLS_ASIDE": "0"}, {"MEMVUL_QKV_ASIDE": "q"}], ids=["cls_aside_0", "qkv_aside_q"])
def test_switches_that_change_the_form_fall_back(env):
    pair = Pair(env)
    try:
        check(pair, 256, lengths(3, 256, seed=9), fixed_applies=False, seed=9)
    finally:
        pair.close()


@pytest.mark.parametrize("bad", ["Fixed", "", "1"])
def test_a_bad_value_of_the_switch_is_refused_at_create(bad):
    with pytest.raises(RuntimeError, match="MEMVUL_PP_FORM"):
        make_engine(bad, {}, 4096)


@pytest.mark.parametrize("M", [256, 768])
def test_the_gemm_hook_is_the_same_under_both_values(default_pair, M):
    rng = np.random.default_rng(M)
    A = rng.standard_normal((M, 768)).astype(np.float32)
    W = (rng.standard_normal((3072, 768)) * 0.05).astype(np.float32)
    bias = rng.standard_normal(3072).astype(np.float32)
    outs = []
    for eng in (default_pair.fixed, default_pair.runtime):
        eng.pp_fixed_launches(reset=True)
        o16, o8, _ = eng.test_gemm_pp(A, W, bias, x8=2)
        assert eng.pp_fixed_launches() == 0  # (the hook's launch is not of the fixed form: see the module's docstring)
        outs.append((o16.tobytes(), o8.tobytes()))
    assert outs[0] == outs[1]
