"""The UTF-8 mode of the device WordPiece tokenizer (include/memvul_hip.h mv_tok_set_unicode / mv_tok_encode_u8*, memvul_amd/csrc/wordpiece.h), the parts that
need no GPU: the rule through its host restatement (mv_tok_encode_u8_host) byte-equal to ``backend_tokenizer.encode_batch`` of the installed ``tokenizers`` on
the edge table and both fuzz sets, for an uncased, a cased and the big vocabulary with non-ASCII pieces; the status rows against the Python rule of
tests/wordpiece_utf8_kit.py; the code-point table against a naive build; the refusals; the Python plumbing of ``batch_ids`` with
``attach_device(unicode=True)``; the switch; and the stand-alone program tools/wordpiece_utf8_host_check.cpp.

The combinations (input bytes, output code points, classes two bits each) of the covered entries, as code_point_table gives them with tokenizers 0.22.2 and
Python 3.10's unicodedata (the test prints them): uncased 83 900 covered code points in 15 combinations — 2 bytes: 310 removed, 1 whitespace, 52 punctuation,
1 498 one word character; 3 bytes: 7 151 removed, 17 whitespace, 523 punctuation, 12 939 one word character, 422 two word characters, 28 053 space + word +
space (CJK), 10 773 three word characters (Hangul); 4 bytes: 352 removed, 123 punctuation, 21 680 one word character, 6 two word characters.  Cased: 83 182 in 12
(no accent stripping, so no entry of two word characters and no Hangul decomposition)."""
import ctypes as C
import os
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
import wordpiece_utf8_kit as u8  # noqa: E402

NAMES = ("mv_tok_set_unicode", "mv_tok_encode_u8", "mv_tok_encode_u8_host")


@pytest.fixture(scope="module")
def lib():
    from memvul_amd import build

    build.build(verbose=False)
    return binding.load_library()


@pytest.fixture(scope="module", params=["small", "big", "cased"])
def rig(request, lib):
    """(name, BertTokenizerFast, DeviceWordPiece without a device and with the table, the Python rule, the table, cased)."""
    cased = request.param == "cased"
    hf = kit.hf_tokenizer(u8.vocab_list(request.param), cased)
    dwp, lits, table = u8.device_wordpiece(hf)
    yield request.param, hf, dwp, u8.Rule(hf, lits), table, cased
    dwp.close()


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_carry_the_entries(lib):
    declared = test_abi._declared_symbols()
    for name in NAMES:
        assert name in declared and name in binding.ABI_SYMBOLS and hasattr(lib, name), name
    vp = C.c_void_p
    assert lib.mv_tok_encode_u8.argtypes == lib.mv_tok_encode_u8_host.argtypes == lib.mv_tok_encode.argtypes
    assert lib.mv_tok_set_unicode.argtypes == [vp, vp, C.c_int]
    assert binding.CODE_POINT_DTYPE.itemsize == 16 and binding.CODE_POINTS == 0x20000


@pytest.mark.parametrize("fn", ["mv_tok_encode_u8_host", "mv_tok_encode_u8"])
def test_bad_arguments_and_a_missing_table_leave_the_outputs_untouched(lib, fn):
    hf = kit.hf_tokenizer(u8.vocab_list("small"))
    bare, _ = kit.device_wordpiece(hf)
    with_table, _, _ = u8.device_wordpiece(hf)
    text, good = b"ab heap", np.array([0, 2, 7], np.int64)
    ids, lens, status = np.full((2, 8), 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.uint8)

    def raw(dwp, t, off, n, ml):
        return getattr(lib, fn)(dwp._t, t, binding._ptr(off) if off is not None else None, n, ml, 1, binding._ptr(ids), binding._ptr(lens), binding._ptr(status))

    cases = [(text, np.array([0, 5, 2], np.int64), 2, 8), (text, np.array([-1, 2, 7], np.int64), 2, 8), (text, good, 2, 1), (text, good, 2, 513), (text, good, -1, 8),
             (None, good, 2, 8), (text, None, 2, 8)]
    for dwp in (bare, with_table):
        for t, off, n, ml in cases:
            assert raw(dwp, t, off, n, ml) == -1, (t, off, n, ml)
            assert lib.mv_tok_last_error(dwp._t)
        assert raw(dwp, text, good, 0, 8) == 0
    assert getattr(lib, fn)(None, text, binding._ptr(good), 2, 8, 1, binding._ptr(ids), binding._ptr(lens), binding._ptr(status)) == -1
    assert raw(bare, text, good, 2, 8) == -3 and b"mv_tok_set_unicode" in lib.mv_tok_last_error(bare._t)  # no table: a state error
    assert (ids == 77).all() and (lens == 77).all() and (status == 77).all()
    if fn == "mv_tok_encode_u8":  # with a table but without a device: a state error as well
        assert raw(with_table, text, good, 2, 8) == -3 and (ids == 77).all() and (lens == 77).all() and (status == 77).all()
    else:
        assert raw(with_table, text, good, 2, 8) == 0 and lens.tolist() == [3, 3] and status.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="mv_tok_encode_u8_host failed"):
        bare.encode_u8_host(*kit.pack([b"ab"]), 8)
    bare.close()
    with_table.close()


def test_the_ascii_entries_do_not_change_on_an_object_with_a_table(rig):
    name, hf, dwp, rule, table, cased = rig
    bare, lits = kit.device_wordpiece(hf)
    rows = kit.edge_rows(cased) + [b"ab\x80", b"\x80", "café".encode(), b"see [SEP] here"]
    got = kit.check(dwp.encode_host, hf, rows, 256, True, lits, name)
    assert got[2][-4:].tolist() == [1, 1, 1, 1] and _same(got, bare.encode_host(*kit.pack(rows), 256, True))
    bare.close()


def test_set_unicode_refuses_malformed_tables(lib):
    hf = kit.hf_tokenizer(u8.vocab_list("small"))
    dwp, _, table = u8.device_wordpiece(hf)
    want = dwp.encode_u8_host(*kit.pack(["straße 가".encode()]), 8)

    def edited(cp, **fields):
        t = table.copy()
        for k, v in fields.items():
            t[k][cp] = v
        return t

    sharp_s = 0xDF
    assert table["covered"][sharp_s] == 1 and bytes(table["out"][sharp_s][:2]) == "ß".encode()
    bad = [edited(sharp_s, nbytes=13), edited(sharp_s, out=np.frombuffer(b"\xc3x" + bytes(10), np.uint8)), edited(sharp_s, out=np.frombuffer(b"\xed\xa0\x80" + bytes(9), np.uint8), nbytes=3),
           edited(sharp_s, cls=0), edited(sharp_s, nchars=2), edited(sharp_s, covered=2), edited(sharp_s, nbytes=1)]
    for t in bad:
        with pytest.raises(RuntimeError, match=r"mv_tok_set_unicode failed \(-1\)"):
            dwp.set_unicode(t)
        assert _same(want, dwp.encode_u8_host(*kit.pack(["straße 가".encode()]), 8))  # the object keeps the table it had
    assert lib.mv_tok_set_unicode(dwp._t, None, 16) == -1 and lib.mv_tok_set_unicode(dwp._t, binding._ptr(table.view(np.uint8)), 0) == -1
    assert lib.mv_tok_set_unicode(dwp._t, binding._ptr(table.view(np.uint8)), 0x20001) == -1 and lib.mv_tok_set_unicode(None, binding._ptr(table.view(np.uint8)), 16) == -1
    with pytest.raises(ValueError):
        dwp.set_unicode(np.zeros((4, 8), np.uint8))
    dwp.close()
    # the word buffer is sized from the rule: 4 bytes x max_chars characters + one step's largest output (67 x the table's largest ratio, 3 for Hangul) must
    # fit 640 bytes — 100 characters do, 190 (what mv_tok_create takes for the ASCII rule) do not
    spec = kit.wrap(hf).device_spec()
    wide = binding.DeviceWordPiece(device=None, **dict(spec, max_chars_per_word=190))
    with pytest.raises(RuntimeError, match="do not fit"):
        wide.set_unicode(table)
    wide.close()
    step = 67 * 3
    assert 4 * 100 + step <= 640 < 4 * 190 + step and (table["nbytes"][0xAC01], table["nchars"][0xAC01]) == (9, 3)
    short = binding.DeviceWordPiece(device=None, **spec)
    short.set_unicode(table[:0x1100])  # code points from n_entries on are uncovered
    assert short.encode_u8_host(*kit.pack(["ß".encode(), "가".encode()]), 8)[2].tolist() == [0, 2]
    short.close()


def test_added_tokens_with_bytes_above_0x7f_are_matched_on_the_raw_bytes(lib):
    """A tokenizer whose added tokens hold bytes >= 0x80 (add_special_tokens with an arrow, a guillemet-quoted word, "k" + e acute): the Rust backend cuts them out
    of the raw text before it normalises — the premise below, on the reference — so a row that holds one is status 1 under the UTF-8 rule; the ASCII rule hands such
    a row back for its bytes anyway."""
    hf = u8.hf_with_added_tokens()
    plain = kit.hf_tokenizer(u8.vocab_list("small"))
    a, b = u8.reference(hf, ["a\u2192b heap".encode()], 8)[0], u8.reference(plain, ["a\u2192b heap".encode()], 8)[0]
    v = plain.get_vocab()
    assert b[0, 1:4].tolist() == [v["a"], v["##\u2192"], v["##b"]] and a[0, 1:4].tolist() == [v["a"], v["\u2192"], v["b"]]  # cut out: other ids
    dwp, lits, table = u8.device_wordpiece(hf)
    assert sorted(lits) == sorted(kit.SPECIALS + u8.ADDED)
    rule = u8.Rule(hf, lits)
    rows, want = u8.added_token_rows()
    assert rule.statuses(rows).tolist() == want
    for ml in (4, 256):
        ids, lens, status = u8.check(dwp.encode_u8_host, hf, rule, rows, ml, True, "added tokens")
        assert status.tolist() == want and not lens[status != 0].any() and not ids[status != 0].any()
    kit.check(dwp.encode_host, hf, rows + kit.edge_rows()[:140], 256, True, lits, "added tokens, the ASCII rule")
    u8.check(dwp.encode_u8_host, hf, rule, list(u8.fuzz_covered()[:300]) + u8.edge_rows(table)[:200], 256, True, "added tokens, fuzz")
    dwp.close()
    # through batch_ids: the rows come back as `literal` and the arrays are the host path's
    host, dev = u8.wrap(hf, 64), u8.wrap(hf, 64).attach_device(0, host_restatement=True, unicode=True)
    texts = [r.decode() for r in rows[:6] + rows[8:14]]
    x, y = host.batch_ids(texts), dev.batch_ids(texts)
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and dev.device_counts == {"device": 6, "literal": 6, "non_ascii": 0}
    dev.detach_device()


def test_a_code_point_the_table_marks_uncovered_is_handed_back(lib):
    """"The table marks it uncovered", apart from how code_point_table decides it: covered = 0 written into an otherwise valid entry; and the two reasons that do
    not occur under BertNormalizer — an output of more than 3 code points, a pre-tokenizer probe that is none of the three patterns — through code_point_table
    over a stand-in normalizer / pre-tokenizer."""
    from memvul_amd.tokenizer import code_point_table

    hf = kit.hf_tokenizer(u8.vocab_list("small"))
    dwp, lits, table = u8.device_wordpiece(hf)
    rows = ["stra\u00dfe".encode(), "caf\u00e9".encode(), b"heap"]
    assert dwp.encode_u8_host(*kit.pack(rows), 16)[2].tolist() == [0, 0, 0]
    edited = table.copy()
    edited["covered"][0xDF] = 0
    dwp.set_unicode(edited)
    ids, lens, status = dwp.encode_u8_host(*kit.pack(rows), 16)
    assert status.tolist() == [2, 0, 0] and lens[0] == 0 and not ids[0].any()
    dwp.set_unicode(table)
    assert dwp.encode_u8_host(*kit.pack(rows), 16)[2].tolist() == [0, 0, 0]

    class _Normalizer:
        def normalize_str(self, s):
            return {"\u00e9": "abcd", "\U00010000": "\U0001f600" * 3, "\u00eb": "\U0001f600" * 4}.get(s, s)

    class _PreTokenizer:
        def pre_tokenize_str(self, s):
            c = s[1:-1]
            return [("a", (0, 1)), (c + "a", (1, len(s)))] if c == "\u00ec" else [("a", (0, 1)), ("a", (2, 3))] if c == "\u00a0" else [(s, (0, len(s)))]

    class _Backend:
        normalizer, pre_tokenizer = _Normalizer(), _PreTokenizer()

    odd = code_point_table(_Backend)
    assert odd["covered"][[0xE8, 0xE9, 0x10000, 0xEB, 0xEC, 0xA0]].tolist() == [1, 0, 1, 0, 0, 1]  # 4 code points / 12 bytes fit / 16 bytes / an unknown pattern / whitespace
    assert (odd["nbytes"][0x10000], odd["nchars"][0x10000], odd["cls"][0x10000], odd["cls"][0xA0]) == (12, 3, 0x3F, 1)
    assert [u8.naive_entry(_Backend, cp)[1] for cp in (0xE9, 0xEB, 0xEC)] == ["size", "size", "probe"]
    dwp.set_unicode(odd)
    got = dwp.encode_u8_host(*kit.pack([chr(c).encode() for c in (0xE8, 0xE9, 0x10000, 0xEB, 0xEC, 0xA0)]), 16)
    assert got[2].tolist() == [0, 2, 0, 2, 2, 0] and got[1].tolist() == [3, 0, 5, 0, 0, 2]
    dwp.close()


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_table_equals_a_naive_build_on_sampled_code_points(rig):
    name, hf, dwp, rule, table, cased = rig
    assert table.dtype == binding.CODE_POINT_DTYPE and table.shape == (0x20000,) and not table[:0x80].view(np.uint8).any()
    rng = np.random.default_rng(5)
    sample = sorted(set(rng.integers(0x80, 0x20000, size=2000).tolist()) | {ord(c) for f in u8.FRAGMENTS for c in f if ord(c) >= 0x80} | {0xD800, 0xDFFF, 0x1FFFF})
    for cp in sample:
        entry, why = u8.naive_entry(hf.backend_tokenizer, cp)
        e = table[cp]
        if entry is None:
            assert not e.tobytes().strip(b"\0"), (hex(cp), why)
            continue
        out, classes = entry
        assert e["covered"] == 1 and e["nbytes"] == len(out) and bytes(e["out"][:len(out)]) == out and not e["out"][len(out):].any(), hex(cp)
        assert e["nchars"] == len(classes) and e["cls"] == sum(k << (2 * j) for j, k in enumerate(classes)), hex(cp)
    combos = u8.combinations(table)
    print(name, int(table["covered"].sum()), "covered;", {k: v[0] for k, v in combos.items()})
    assert {k[0] for k in combos} == {2, 3, 4} and {k[1] for k in combos} >= {0, 1, 3}
    assert (table["nbytes"] <= 12).all() and (table["nchars"] <= 3).all()


def test_the_kernel_library_is_fingerprinted_like_the_main_one(lib):
    """wp_encode_u8_kernel lives in libmemvul_tok_u8.so, outside the kernel map of libmemvul_hip.so that the pass fingerprints are keyed on: its own map is
    recorded in profiles/kernel_fingerprints_tok.json, so a change to the kernel shows as a changed hash (python scripts/kernel_fingerprints.py --tok --out
    profiles/kernel_fingerprints_tok.json records it again); the main library holds no UTF-8 kernel, the new library nothing else."""
    import json

    from memvul_amd import build

    fp = build.kernel_fingerprints(build.LIB_PATH_TOK)
    assert sorted(k for k in fp if not k.endswith(".kd")) == [k for k in fp if "wp_encode_u8_kernel" in k and not k.endswith(".kd")] and len(fp) == 2
    assert not any("wp_encode_u8" in k for k in build.kernel_fingerprints()) and any("wp_encode_kernel" in k for k in build.kernel_fingerprints())
    with open(os.path.join(ROOT, "profiles", "kernel_fingerprints_tok.json")) as f:
        assert json.load(f) == fp, "the UTF-8 kernel changed: record profiles/kernel_fingerprints_tok.json again (scripts/kernel_fingerprints.py --tok --out)"


# ---- the rule, through the host restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("add_special", [True, False])
@pytest.mark.parametrize("max_length", u8.MAX_LENGTHS)
def test_edge_table_equals_the_rust_tokenizer(rig, max_length, add_special):
    name, hf, dwp, rule, table, cased = rig
    rows = u8.edge_rows(table, cased) + u8.truncation_rows(max_length, add_special)
    ids, lens, status = u8.check(dwp.encode_u8_host, hf, rule, rows, max_length, add_special, name)
    ascii_rows = [i for i, r in enumerate(rows) if r.isascii()]
    assert len(ascii_rows) > 150 and not status[ascii_rows].any()
    old = dwp.encode_host(*kit.pack([rows[i] for i in ascii_rows]), max_length, add_special)  # the ASCII rows: the ASCII path's ids
    assert _same((ids[ascii_rows], lens[ascii_rows], status[ascii_rows]), old)


def test_the_edge_rows_are_what_they_claim(rig):
    """The table's premises, on the reference alone."""
    name, hf, dwp, rule, table, cased = rig
    v, unk = hf.get_vocab(), hf.unk_token_id
    rows = ["q" * 99 + "ß", "q" * 100 + "ß", "ß" * 100, "ß" * 101, "\U0001f600" * 100, "\U0001f600" * 101, "ab\u200bab", "abab", "ab\u00adab",
            "café", "ab中ab", "가", "İ", "straße", "€→"]
    ids, lens = u8.reference(hf, [r.encode() for r in rows], 256)
    assert ids[0, 1] == v[u8.LONG_U8] and lens[0] == 3  # 100 characters in 101 bytes are looked up: the limit counts characters
    assert ids[1, 1] == unk and lens[1] == 3
    assert lens[2] == 102 and unk not in ids[2, :102].tolist() and ids[3, 1] == unk and lens[3] == 3  # 100 pieces / one [UNK]
    assert lens[4] == 102 and ids[5, 1] == unk and lens[5] == 3
    assert ids[6].tolist() == ids[7].tolist() == ids[8].tolist()  # zero width space and soft hyphen are removed: their neighbours join
    assert v["中"] in ids[10, 2:lens[10] - 2].tolist() and ids[14, 1:3].tolist() == [v["€"], v["##→"]]  # a CJK character inside a word is a word of its own
    if name == "big":  # (the synthetic big vocabulary has other ASCII pieces)
        return
    assert ids[10, 1:4].tolist() == [v["ab"], v["中"], v["ab"]] and lens[13] == 8 and unk not in ids[13, :8].tolist()
    if cased:
        assert ids[9, 1:4].tolist() == [v["c"], v["##a"], v["##f"]] and ids[9, 4] == v["##é"] and ids[11, 1] == unk
    else:
        assert ids[9, 1] == v["cafe"] and lens[9] == 3  # the accent is stripped and the word becomes a vocabulary word
        assert ids[11, 1:3].tolist() == [v["ᄀ"], v["##ᅡ"]] and ids[12, 1] == v["i"]  # Hangul decomposes; I with dot above ends as i


def test_status_rows(rig):
    name, hf, dwp, rule, table, cased = rig
    rows, want = u8.status_rows(rule)
    reasons = u8.uncovered_examples(rule)
    assert {"unassigned", "combining"} <= set(reasons), reasons  # (no entry exceeds 3 code points or 12 bytes and no probe shows a fourth pattern with this tokenizer)
    assert rule.statuses(rows).tolist() == want  # the Python rule agrees with the premises written beside the rows
    for ml in (4, 256):
        ids, lens, status = u8.check(dwp.encode_u8_host, hf, rule, rows, ml, True, name)
        assert status.tolist() == want
        assert not lens[status != 0].any() and not ids[status != 0].any()


@pytest.mark.parametrize("which", ["covered", "stray"])
def test_fuzz_equals_the_rust_tokenizer(rig, which):
    name, hf, dwp, rule, table, cased = rig
    texts = list(u8.fuzz_covered(cased) if which == "covered" else u8.fuzz_stray(cased))
    want = rule.statuses(texts)
    assert len(texts) == 2000 and max(map(len, texts)) <= 3000 and sum(not t.isascii() for t in texts) > 1500
    if which == "covered":  # on the Python rule alone: nothing hides behind a hand-back
        assert not want.any()
    else:
        assert not (want == 1).any() and 0.05 <= (want == 2).mean() <= 0.40, (want == 2).mean()
    ids, lens, status = u8.check(dwp.encode_u8_host, hf, rule, texts, 256, True, name + " " + which)
    assert lens[status == 0].min() >= 2 and lens.max() == 256


# ---- Python plumbing ----------------------------------------------------------------------------------------------------------------------------------------------

def test_batch_ids_with_unicode_attached_equals_the_host_path(lib):
    from test_device_wordpiece_cpu import MIXED

    hf = kit.hf_tokenizer(u8.vocab_list("small"))
    mixed = MIXED + ["straße €5 a→b", "\U00020000 beyond the table", "\u0378 unassigned", "\U0001f600 [SEP]"]
    for max_length, add_special in ((256, True), (12, True), (12, False)):
        plain, dev = u8.wrap(hf, max_length, add_special), u8.wrap(hf, max_length, add_special)
        dev.attach_device(0, host_restatement=True, unicode=True)
        for texts in (mixed, mixed[:1], [mixed[2]], ["", ""], [t for t in mixed if t.isascii()], [t for t in mixed if not t.isascii()]):
            a, b = plain.batch_ids(texts), dev.batch_ids(texts)
            assert a[0].dtype == b[0].dtype == np.int32 and a[0].shape == b[0].shape and a[0].flags.c_contiguous and b[0].flags.c_contiguous
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and b[1].dtype == np.int32
        dev.detach_device()
    dev = u8.wrap(hf, 256, True)
    assert dev.device_unicode_rows == 0
    dev.attach_device(0, host_restatement=True, unicode=True)
    table = dev._code_points
    dev.batch_ids(mixed)
    rule = u8.Rule(hf)
    want = rule.statuses([t.encode() for t in mixed])
    n1, n2 = int((want == 1).sum()), int((want == 2).sum())
    assert (n1, n2) == (4, 2)
    assert dev.device_counts == {"device": len(mixed) - n1 - n2, "literal": n1, "non_ascii": n2}
    assert dev.device_unicode_rows == sum((not t.isascii()) and w == 0 for t, w in zip(mixed, want)) == 3
    # a lone surrogate is no UTF-8: it reaches the device as a malformed sequence, comes back, and the Rust tokenizer decides as on the host path
    lone = ["ab \ud800 cd", "plain"]
    outcome = []
    for t in (u8.wrap(hf, 256, True), dev):
        try:
            outcome.append(tuple(x.tobytes() for x in t.batch_ids(lone)))
        except Exception as e:  # noqa: BLE001 - both paths must fail alike
            outcome.append(type(e))
    assert outcome[0] == outcome[1], outcome
    # the table is built once per tokenizer object; attaching without unicode afterwards is the ASCII mode again
    dev.attach_device(0, host_restatement=True, unicode=True)
    assert dev._code_points is table
    dev.attach_device(0, host_restatement=True)
    dev.device_counts = {"device": 0, "literal": 0, "non_ascii": 0}
    dev.batch_ids(mixed)
    assert dev.device_counts["non_ascii"] == sum(not t.isascii() for t in mixed) and dev._device_unicode is False
    dev.detach_device()


def test_the_switch_takes_gpu_utf8(monkeypatch):
    assert binding.TOKENIZE_MODES == ("host", "gpu", "gpu-utf8")
    monkeypatch.setenv("MEMVUL_TOKENIZE", "gpu-utf8")
    assert binding.tokenize_policy() == "gpu-utf8" and binding.tokenize_policy("gpu-utf8") == "gpu-utf8" and binding.tokenize_policy("host") == "host"
    for typo in ("gpu_utf8", "gpu-utf-8", "GPU-UTF8", "gpu-utf8 "):
        with pytest.raises(ValueError, match="tokenize"):
            binding.tokenize_policy(typo)
        monkeypatch.setenv("MEMVUL_TOKENIZE", typo)
        with pytest.raises(ValueError, match="MEMVUL_TOKENIZE"):
            binding.tokenize_policy()
    from memvul_amd import predict_memory as pm

    seen = {}

    class _Tok:
        def attach_device(self, index, unicode=False):
            seen.update(index=index, unicode=unicode)

    class _Archive:
        class dataset_reader:
            _tokenizer = _Tok()

        class model:
            _device_index = 3
    assert pm.attach_tokenizer(_Archive, {"tokenize": "gpu-utf8"}) is True and seen == {"index": 3, "unicode": True}
    assert pm.attach_tokenizer(_Archive, {"tokenize": "gpu"}) is True and seen == {"index": 3, "unicode": False}


# ---- the stand-alone check of the host core ------------------------------------------------------------------------------------------------------------------------

def test_host_core_program_agrees_with_a_naive_restatement(tmp_path):
    """tools/wordpiece_utf8_host_check.cpp: a stand-alone program (its own main, nothing loaded into python) over the UTF-8 host core of wordpiece.h — decode,
    table check, matcher at character boundaries, wp_encode_text_u8 — against a naive restatement, built with -fsanitize=address,undefined (its header comment
    gives the line)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "wordpiece_utf8_host_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "memvul_amd", "csrc"),
                            os.path.join(ROOT, "tools", "wordpiece_utf8_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]  # the sanitized build or none: a run that passes has run under the sanitizers
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))  # (the leak check needs ptrace, which a container may deny)
    assert run.returncode == 0 and "wordpiece_utf8_host_check: OK" in run.stdout, (run.stdout[-1000:], run.stderr[-2000:])
