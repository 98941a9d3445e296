"""The device WordPiece tokenizer (include/memvul_hip.h mv_tok_*, memvul_amd/csrc/wordpiece.h), the parts that need no GPU: the ABI in header, binding and
exports; the rule through its host restatement (mv_tok_encode_host) byte-equal to ``backend_tokenizer.encode_batch`` of the installed ``tokenizers`` on the
edge table and both fuzz sets; the status rows; the Python plumbing of ``batch_ids`` with the host restatement injected; the refusals of ``attach_device``;
the switch; and the stand-alone program of tools/wordpiece_host_check.cpp (built plainly here; its sanitizer run is recorded in
profiles/wordpiece_host_check_sanitizers.txt)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from memvul_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_abi  # noqa: E402
import wordpiece_kit as kit  # noqa: E402

NAMES = ("mv_tok_create", "mv_tok_encode", "mv_tok_encode_host", "mv_tok_kernel_ms", "mv_tok_destroy", "mv_tok_last_error")


@pytest.fixture(scope="module")
def lib():
    from memvul_amd import build

    build.build(verbose=False)
    return binding.load_library()


@pytest.fixture(scope="module", params=["small", "big", "cased"])
def rig(request, lib):
    """(name, BertTokenizerFast, DeviceWordPiece without a device, literals, cased)."""
    cased = request.param == "cased"
    toks = kit.big_vocab_list()[0] if request.param == "big" else kit.small_vocab_list(cased)
    assert len(toks) == (30522 if request.param == "big" else 150)
    hf = kit.hf_tokenizer(toks, cased)
    dwp, lits = kit.device_wordpiece(hf)
    yield request.param, hf, dwp, lits, cased
    dwp.close()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_carry_the_entries(lib):
    declared = test_abi._declared_symbols()
    hdr = open(os.path.join(ROOT, "include", "memvul_hip.h")).read()
    from stage_kit import host_source

    src = host_source()
    for name in NAMES:
        assert name in declared and name in binding.ABI_SYMBOLS and hasattr(lib, name), name
    assert declared == sorted(binding.ABI_SYMBOLS)
    vp = C.c_void_p
    assert lib.mv_tok_create.argtypes == [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    assert lib.mv_tok_encode.argtypes == lib.mv_tok_encode_host.argtypes == [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    assert lib.mv_tok_destroy.argtypes == [vp] and lib.mv_tok_destroy.restype is None
    assert lib.mv_tok_last_error.argtypes == [vp] and lib.mv_tok_last_error.restype == C.c_char_p
    assert "typedef struct mv_tokenizer mv_tokenizer;" in hdr
    for name in ("mv_tok_create", "mv_tok_encode", "mv_tok_encode_host"):  # function-try-blocks like every other entry (test_abi checks the whole file)
        assert re.search(r"^int %s\([^{;]*\) try \{" % name, src, flags=re.M), name
    assert "struct mv_tokenizer {" in src and "mv_tokenizer" not in src[src.index("struct mv_handle {"):src.index("\n};\n", src.index("struct mv_handle {"))]  # not part of a handle (the struct's own text)


def _raw(lib, dwp, fn, text, off, n, max_length, ids, lens, status):
    return getattr(lib, fn)(dwp._t, text, binding._ptr(off) if off is not None else None, n, max_length, 1, binding._ptr(ids), binding._ptr(lens), binding._ptr(status))


@pytest.mark.parametrize("fn", ["mv_tok_encode_host", "mv_tok_encode"])
def test_bad_arguments_leave_the_outputs_untouched(lib, fn):
    dwp, _ = kit.device_wordpiece(kit.hf_tokenizer(kit.small_vocab_list()))
    text, good = b"ab heap", np.array([0, 2, 7], np.int64)
    ids, lens, status = np.full((2, 8), 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.uint8)
    cases = [(text, np.array([0, 5, 2], np.int64), 2, 8), (text, np.array([-1, 2, 7], np.int64), 2, 8), (text, good, 2, 1), (text, good, 2, 513), (text, good, -1, 8),
             (None, good, 2, 8), (text, None, 2, 8)]
    for t, off, n, ml in cases:
        assert _raw(lib, dwp, fn, t, off, n, ml, ids, lens, status) == -1, (t, off, n, ml)
        assert lib.mv_tok_last_error(dwp._t)
    for out in ("ids", "lens", "status"):
        args = dict(ids=ids, lens=lens, status=status)
        args[out] = None
        assert getattr(lib, fn)(dwp._t, text, binding._ptr(good), 2, 8, 1, binding._ptr(args["ids"]), binding._ptr(args["lens"]), binding._ptr(args["status"])) == -1
    assert (ids == 77).all() and (lens == 77).all() and (status == 77).all()
    assert getattr(lib, fn)(None, text, binding._ptr(good), 2, 8, 1, binding._ptr(ids), binding._ptr(lens), binding._ptr(status)) == -1
    assert _raw(lib, dwp, fn, text, good, 0, 8, ids, lens, status) == 0 and (ids == 77).all()  # n == 0: MV_OK, nothing read or written — also without a device
    if fn == "mv_tok_encode":  # an object created without a device has no kernel to run: a state error, outputs untouched
        assert _raw(lib, dwp, fn, text, good, 2, 8, ids, lens, status) == -3 and (ids == 77).all() and (lens == 77).all() and (status == 77).all()
    else:
        assert _raw(lib, dwp, fn, text, good, 2, 8, ids, lens, status) == 0 and lens.tolist() == [3, 3] and status.tolist() == [0, 0]
    dwp.close()


def test_create_refuses_bad_tables(lib):
    t = C.c_void_p()
    vb, vo = binding._packed([b"[UNK]", b"[CLS]", b"[SEP]", b"ab"])
    lb, lo = binding._packed([b"[SEP]"])
    for unk, mc, lo_ in ((9, 100, lo), (0, 0, lo), (0, 191, lo), (0, 100, np.array([0, 0], np.int64))):
        assert lib.mv_tok_create(-1, vb, binding._ptr(vo), 4, lb, binding._ptr(lo_), 1, unk, 1, 2, mc, 1, C.byref(t)) == -1 and not t.value
        assert lib.mv_tok_last_error(None)
    with pytest.raises(RuntimeError, match="mv_tok_create"):
        binding.DeviceWordPiece([b"a"], [], 5, 0, 0, device=None)


# ---- the rule, through the host restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("add_special", [True, False])
@pytest.mark.parametrize("max_length", kit.MAX_LENGTHS)
def test_edge_table_equals_the_rust_tokenizer(rig, max_length, add_special):
    name, hf, dwp, lits, cased = rig
    kit.check(dwp.encode_host, hf, kit.edge_rows(cased) + kit.truncation_rows(max_length, add_special), max_length, add_special, lits, name)


def test_the_edge_rows_are_what_they_claim(rig):
    """The table's premises, on the reference alone: the 100-character word is looked up, 101 characters are [UNK], an unmatched tail makes the WHOLE word
    [UNK], a removed byte joins its neighbours."""
    name, hf, dwp, lits, cased = rig
    ids, lens = kit.reference(hf, [b"q" * 100, b"q" * 101, b"ab\x01ab", b"abab", b"ab ab"], 16)
    unk, long_id = hf.unk_token_id, hf.get_vocab()[kit.LONG_WORD]
    assert ids[0, :3].tolist() == [hf.cls_token_id, long_id, hf.sep_token_id] and ids[1, 1] == unk and lens[1] == 3
    assert ids[2].tolist() == ids[3].tolist() != ids[4].tolist()
    if name != "big":  # (no 'z' in the small vocabularies)
        ids, lens = kit.reference(hf, [b"bufferz", b"buffer"], 16)
        assert lens.tolist() == [3, 3] and ids[0, 1] == unk and ids[1, 1] != unk


def test_status_rows(rig):
    name, hf, dwp, lits, cased = rig
    assert sorted(lits) == sorted(kit.SPECIALS)  # read from the serialised tokenizer, not hard-coded: what this vocabulary's BertTokenizerFast adds
    rows, want = [], []
    for l in lits:
        lb = l.encode()
        rows += [lb + b" heap", b"see " + lb + b" here", b"see" + lb + b"here", lb, b"a" * 300 + lb]
        want += [1] * 5
    rows += [b"[sep]", b"[CLS", b"[unused5]", b"[ SEP ]", b"[SE\x01P]", b"CLS] [", b"ab\x80", b"\x80", b"a" * 700 + b"\xc3\xa9"]
    want += [0, 0, 0, 0, 0, 0, 1, 1, 1]
    for ml in (4, 256):
        ids, lens, status = kit.check(dwp.encode_host, hf, rows, ml, True, lits, name)
        assert status.tolist() == want
        assert not lens[status == 1].any() and not ids[status == 1].any()
    # the premise, on the reference: an added token is cut out of the raw text — glued to a word, and case-sensitively
    ids, _ = kit.reference(hf, [b"see[MASK]here", b"[sep]"], 16)
    assert hf.mask_token_id in ids[0].tolist() and hf.sep_token_id not in ids[1, 1:4].tolist()


@pytest.mark.parametrize("which", ["bytes", "corpus"])
def test_fuzz_equals_the_rust_tokenizer(rig, which):
    name, hf, dwp, lits, cased = rig
    texts = list(kit.fuzz_bytes() if which == "bytes" else kit.fuzz_corpus())
    assert len(texts) == 2000
    if which == "bytes":
        seen = np.zeros(128, bool)
        seen[np.frombuffer(b"".join(texts), np.uint8)] = True
        assert seen.all() and max(map(len, texts)) <= 3000
    ids, lens, status = kit.check(dwp.encode_host, hf, texts, 256, True, lits, name + " " + which)
    # no row comes back that the substring rule does not name (kit.check compares the status bytes with the literal search); these draws hold none at all
    assert not kit.literal_rows(texts, lits).any() and not status.any()
    assert lens.min() >= 2 and lens.max() == 256


# ---- Python plumbing ----------------------------------------------------------------------------------------------------------------------------------------------

MIXED = ["heap overflow in the parser", "", "café crash", "see [SEP] here", "Buffer\x01ed the STACK", "中文 report", "   ", "null free [MASK]", "ab " * 400,
         "naïve [CLS] both", "plain again", "q" * 101]


def test_batch_ids_with_the_host_restatement_equals_the_host_path(lib):
    hf = kit.hf_tokenizer(kit.small_vocab_list())
    for max_length, add_special in ((256, True), (12, True), (12, False)):
        plain, dev = kit.wrap(hf, max_length, add_special), kit.wrap(hf, max_length, add_special)
        dev.attach_device(0, host_restatement=True)
        for texts in (MIXED, MIXED[:1], [MIXED[2]], ["", ""], [t for t in MIXED if t.isascii()]):
            a, b = plain.batch_ids(texts), dev.batch_ids(texts)
            assert a[0].dtype == b[0].dtype == np.int32 and a[0].shape == b[0].shape and a[0].flags.c_contiguous and b[0].flags.c_contiguous
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and b[1].dtype == np.int32
        dev.detach_device()
    dev = kit.wrap(hf, 256, True).attach_device(0, host_restatement=True)
    dev.batch_ids(MIXED)
    n_non_ascii = sum(not t.isascii() for t in MIXED)
    n_literal = sum(t.isascii() and any(l in t for l in kit.SPECIALS) for t in MIXED)
    assert (n_non_ascii, n_literal) == (3, 2)
    assert dev.device_counts == {"device": len(MIXED) - n_non_ascii - n_literal, "literal": n_literal, "non_ascii": n_non_ascii}
    dev.batch_ids(MIXED[:2])
    assert dev.device_counts["device"] == len(MIXED) - n_non_ascii - n_literal + 2
    # batch_token_rows / batch_tokenize sit on batch_ids: the same tokens either way
    assert kit.wrap(hf).batch_tokenize(MIXED[:5]) == dev.batch_tokenize(MIXED[:5])
    # without max_length neither the width nor the work per row is bounded: the host path, the counters untouched
    free = kit.wrap(hf, None, True).attach_device(0, host_restatement=True)
    a, b = kit.wrap(hf, None, True).batch_ids(MIXED), free.batch_ids(MIXED)
    assert a[0].tobytes() == b[0].tobytes() and free.device_counts == {"device": 0, "literal": 0, "non_ascii": 0}


def test_attach_device_refuses_what_the_rule_does_not_restate(lib, monkeypatch):
    import json

    from tokenizers import Tokenizer

    from memvul_amd.tokenizer import PretrainedTransformerTokenizer

    hf = kit.hf_tokenizer(kit.small_vocab_list())
    spec = json.loads(hf.backend_tokenizer.to_str())

    def variant(edit):
        d = json.loads(json.dumps(spec))
        edit(d)
        t = kit.wrap(hf)

        class _Hf:
            backend_tokenizer = Tokenizer.from_str(json.dumps(d))
        t._hf = _Hf()
        return t

    with pytest.raises(ValueError, match="normalizer.clean_text"):
        variant(lambda d: d["normalizer"].update(clean_text=False)).attach_device(0, host_restatement=True)
    with pytest.raises(ValueError, match="model.continuing_subword_prefix"):
        variant(lambda d: d["model"].update(continuing_subword_prefix="@@")).attach_device(0, host_restatement=True)
    with pytest.raises(ValueError, match="pre_tokenizer.type"):
        variant(lambda d: d.update(pre_tokenizer={"type": "Whitespace"})).attach_device(0, host_restatement=True)
    with pytest.raises(ValueError, match="normalized"):
        variant(lambda d: d["added_tokens"][4].update(normalized=True)).attach_device(0, host_restatement=True)

    def to_wordlevel(d):
        d["model"] = {"type": "WordLevel", "vocab": d["model"]["vocab"], "unk_token": "[UNK]"}
    with pytest.raises(ValueError, match="model.type"):
        variant(to_wordlevel).attach_device(0, host_restatement=True)
    with pytest.raises(ValueError, match="max_length"):
        kit.wrap(hf, 513).attach_device(0, host_restatement=True)
    # a cased tokenizer is restated (lowercase is read, not assumed)
    assert kit.wrap(kit.hf_tokenizer(kit.small_vocab_list(True), True)).device_spec()["lowercase"] is False and kit.wrap(hf).device_spec()["lowercase"] is True
    assert kit.wrap(hf).device_spec()["max_chars_per_word"] == 100
    # the hashing stand-in has no WordPiece backend at all
    monkeypatch.setenv("MEMVUL_ALLOW_HASH_TOKENIZER", "1")
    monkeypatch.delenv("MEMVUL_BERT_VOCAB", raising=False)
    stand_in = PretrainedTransformerTokenizer("no-such-model-on-disk", max_length=256)
    assert stand_in._hf is None
    with pytest.raises(ValueError, match="hashing stand-in"):
        stand_in.attach_device(0, host_restatement=True)
    assert stand_in._device is None


def test_the_switch_is_parsed_strictly(monkeypatch):
    monkeypatch.delenv("MEMVUL_TOKENIZE", raising=False)
    assert binding.tokenize_policy() == "host"
    monkeypatch.setenv("MEMVUL_TOKENIZE", "gpu")
    assert binding.tokenize_policy() == "gpu" and binding.tokenize_policy("host") == "host"
    monkeypatch.setenv("MEMVUL_TOKENIZE", "gqu")
    with pytest.raises(ValueError, match="MEMVUL_TOKENIZE"):
        binding.tokenize_policy()
    with pytest.raises(ValueError, match="tokenize"):
        binding.tokenize_policy("GPU")
    # the drivers read it where they attach: a typo raises before anything is tokenised, and "host" attaches nothing
    from memvul_amd import predict_memory as pm

    class _Archive:
        class dataset_reader:
            _tokenizer = None
        model = None
    with pytest.raises(ValueError, match="MEMVUL_TOKENIZE"):
        pm.attach_tokenizer(_Archive)
    monkeypatch.setenv("MEMVUL_TOKENIZE", "host")
    assert pm.attach_tokenizer(_Archive) is False
    with pytest.raises(RuntimeError, match="cannot be attached"):
        pm.attach_tokenizer(_Archive, {"tokenize": "gpu"})


# ---- the stand-alone check of the host core ------------------------------------------------------------------------------------------------------------------------

def test_host_core_program_agrees_with_a_naive_restatement(tmp_path):
    """tools/wordpiece_host_check.cpp: a stand-alone program (its own main, nothing loaded into python) over wordpiece.h's host core — the edge rows and 200
    fuzz rows against a naive restatement over std::map.  Built plainly here; its header comment gives the -fsanitize=address,undefined build that is run by
    hand on a development box."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "wordpiece_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "memvul_amd", "csrc"), os.path.join(ROOT, "tools", "wordpiece_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "wordpiece_host_check: OK" in run.stdout, (run.stdout[-1000:], run.stderr[-2000:])
