"""Shared case tables for the UTF-8 mode of the device WordPiece tokenizer (tests/test_device_wordpiece_utf8_cpu.py, tests/test_device_wordpiece_utf8_gpu.py),
on top of tests/wordpiece_kit.py.  THE REFERENCE of every id comparison is ``backend_tokenizer.encode_batch`` of the installed ``tokenizers``; THE REFERENCE
of every status byte is ``Rule`` below: Python's own strict UTF-8 decoder, a substring search for the added-token literals and a naive, code point by code
point restatement of the coverage rule — never the code under test, and not memvul_amd.tokenizer.code_point_table either."""
import functools
import unicodedata

import numpy as np

import wordpiece_kit as kit

LONG_U8 = "q" * 99 + "ß"  # 100 characters, 101 bytes: still looked up, because max_input_chars_per_word counts characters
PIECES = ["cafe", "ß", "##ß", "€", "##€", "→", "##→", "中", "😀", "##😀", "ᄀ", "##ᅡ", "é", "##é", "##̇", LONG_U8]
MAX_LENGTHS = (2, 3, 8, 256, 512)


def vocab_list(name):
    """The vocabulary of rig ``name`` (small / cased / big): the old kit's plus the non-ASCII pieces."""
    toks = kit.big_vocab_list()[0] if name == "big" else kit.small_vocab_list(name == "cased")
    toks = list(dict.fromkeys(list(toks) + PIECES))
    assert all(p in toks for p in PIECES)
    return toks


def device_wordpiece(hf, device=None):
    """kit.device_wordpiece with the code-point table of ``hf`` attached (built by the code under test: memvul_amd.tokenizer.code_point_table)."""
    from memvul_amd.tokenizer import code_point_table

    dwp, lits = kit.device_wordpiece(hf, device)
    table = code_point_table(hf.backend_tokenizer)
    dwp.set_unicode(table)
    return dwp, lits, table


def wrap(hf, max_length=256, add_special=True):
    """kit.wrap plus what PretrainedTransformerTokenizer.__init__ sets for the UTF-8 mode."""
    t = kit.wrap(hf, max_length, add_special)
    t._device_unicode, t._code_points, t.device_unicode_rows = False, None, 0
    return t


ADDED = ["\u2192", "\u00absep\u00bb", "k\u00e9"]  # added tokens with bytes >= 0x80: a whole character, one between two others, one behind an ASCII first byte


def hf_with_added_tokens(name="small"):
    """The tokenizer of rig ``name`` after add_special_tokens(ADDED): the Rust backend cuts those out of the raw text like [SEP] and [MASK]."""
    hf = kit.hf_tokenizer(vocab_list(name), name == "cased")
    assert hf.add_special_tokens({"additional_special_tokens": ADDED}) == len(ADDED)
    return hf


def added_token_rows():
    """(rows, statuses): rows that hold an added token with bytes >= 0x80 are status 1, on the raw bytes — also beside malformed bytes; near misses are not."""
    rows = ["a\u2192b heap", "\u2192", "see \u00absep\u00bb here", "ok\u00e9", "x" * 300 + "\u2192", "caf\u00e9 \u2192 [MASK]"]
    rows = [r.encode() for r in rows] + [b"\x80\xe2\x86\x92", b"\xe2\x86\x92\xc3"]
    want = [1] * len(rows)
    near = ["k\u00e8 heap", "caf\u00e9 heap", "\u00ab sep \u00bb", "\u00absep", "a\u2190b\u2193", "ke\u0301"]
    rows += [r.encode() for r in near] + [b"ab\xe2\x86"]
    return rows, want + [0] * len(near) + [2]


def naive_entry(bt, cp):
    """The coverage rule for one code point, restated naively: None when uncovered (with the reason as a second value), else (output bytes, classes)."""
    ch = chr(cp)
    if 0xD800 <= cp <= 0xDFFF or unicodedata.category(ch) == "Cn":
        return None, "unassigned"
    out = bt.normalizer.normalize_str(ch)
    if len(out) > 3 or len(out.encode("utf-8")) > 12:
        return None, "size"
    classes = []
    for c in out:
        if unicodedata.combining(c) != 0:
            return None, "combining"
        got = [w for w, _ in bt.pre_tokenizer.pre_tokenize_str("a" + c + "a")]
        if got == ["a", c, "a"]:
            classes.append(2)
        elif got == ["a", "a"]:
            classes.append(1)
        elif got == ["a" + c + "a"]:
            classes.append(3)
        else:
            return None, "probe"
    return (out.encode("utf-8"), classes), None


class Rule:
    """The status byte of a row, in Python: 1 for an added-token literal in the raw bytes, else 2 for bytes Python's strict decoder refuses, a code point
    >= U+20000 or an uncovered one, else 0."""

    def __init__(self, hf, literals=kit.SPECIALS):
        self.bt, self.lit, self._covered = hf.backend_tokenizer, [l.encode() for l in literals], {}

    def covered(self, cp):
        if cp < 0x80:
            return True
        if cp >= 0x20000:
            return False
        got = self._covered.get(cp)
        if got is None:
            got = self._covered[cp] = naive_entry(self.bt, cp)[0] is not None
        return got

    def status(self, row: bytes) -> int:
        if any(l in row for l in self.lit):
            return 1
        if row.isascii():
            return 0
        try:
            text = row.decode("utf-8")
        except UnicodeDecodeError:
            return 2
        return 0 if all(self.covered(ord(c)) for c in set(text)) else 2

    def statuses(self, rows):
        return np.array([self.status(r) for r in rows], np.uint8)


def reference(hf, rows, max_length, add_special=True):
    """ids int32 [n, max_length] zero-padded and lens int32 [n] from the Rust tokenizer; ``rows`` are well-formed UTF-8."""
    bt = hf.backend_tokenizer
    bt.enable_truncation(max_length=max_length)
    bt.no_padding()
    encs = bt.encode_batch([r.decode("utf-8") for r in rows], add_special_tokens=add_special)
    ids, lens = np.zeros((len(rows), max_length), np.int32), np.zeros(len(rows), np.int32)
    for i, e in enumerate(encs):
        lens[i] = len(e.ids)
        ids[i, :len(e.ids)] = e.ids
    return ids, lens


def check(encode, hf, rule, rows, max_length, add_special=True, what=""):
    """``encode`` (DeviceWordPiece.encode_u8 / encode_u8_host) against the references on ``rows`` (bytes): the status bytes are the rule's; rows of status 1 and
    2 have length 0 and a zero id row; every other row is byte-equal to the Rust tokenizer's, padding included.  Returns what ``encode`` returned."""
    ids, lens, status = encode(*kit.pack(rows), max_length, add_special)
    want = rule.statuses(rows)
    assert status.tolist() == want.tolist(), (what, "status", [(int(i), rows[i][:40], int(status[i]), int(want[i])) for i in np.flatnonzero(status != want)[:5]])
    ours = want == 0
    want_ids, want_lens = reference(hf, [r if o else b"" for r, o in zip(rows, ours)], max_length, add_special)
    want_ids[~ours], want_lens[~ours] = 0, 0
    bad = np.flatnonzero((lens != want_lens) | (ids != want_ids).any(1))
    assert not len(bad), (what, max_length, add_special, int(bad[0]), rows[int(bad[0])][:200], ids[bad[0], :16].tolist(), want_ids[bad[0], :16].tolist(),
                          int(lens[bad[0]]), int(want_lens[bad[0]]))
    return ids, lens, status


# ---- the edge table ---------------------------------------------------------------------------------------------------------------------------------------------------

FRAGMENTS = ["caf\u00e9", "stra\u00dfe", "\u20ac5", "a\u2192b", "\u4e2d\u6587", "\ud55c\uad6d\uc5b4", "\uac00", "\u1100", "\u0130", "\u0130stanbul", "\u01c5",
             "\u039f\u0394\u039f\u03a3", "\u03bf\u03b4\u03bf\u03c2", "\u03c2", "ab\u200bab", "ab\u200dab", "ab\u00adab", "\ufeffab", "ab\ufeffab", "\ufb01le",
             "\U0001f600", "a\U0001f600b", "\U0001f600\U0001f600", "\u263a\ufe0f", "ab\ufe0fab", "\u0645\u064f\u062d\u064e\u0645\u0651\u064e\u062f",
             "q" * 99 + "\u00df", "q" * 99 + "\u00e9", "q" * 100 + "\u00df", "q" * 100 + "\u00e9", "\u201cquoted\u201d \u2013 text\u2026 \u2122",
             "na\u00efve \u00fcber \u00dcn\u00efc\u00f6d\u00e9", "ab\u00a0ab", "ab\u3000ab", "ab\u2028ab", "a\u2014b", "\u00bfqu\u00e9?", "x\u00b2", "\u00bd",
             "\u01c6", "\u0149", "\u0390", "\u0130\u0307", "e\u0301"]


def combinations(table):
    """{(input bytes, output code points, packed classes): (count, first code point)} over the covered entries of a code-point table."""
    cps = np.flatnonzero(table["covered"])
    inlen = np.where(cps < 0x800, 2, np.where(cps < 0x10000, 3, 4))
    keys = np.stack([inlen, table["nchars"][cps], table["cls"][cps]], 1)
    uniq, first, counts = np.unique(keys, axis=0, return_index=True, return_counts=True)
    return {tuple(int(x) for x in k): (int(c), int(cps[f])) for k, f, c in zip(uniq, first, counts)}


def edge_rows(table, cased=False):
    """The UTF-8 edge table (bytes): one covered representative of every (input length) x (output code points) x (classes) combination between "ab" and "ab";
    every fragment alone, inside a sentence and glued to ASCII; words of 99 / 100 / 101 characters of 2-, 3- and 4-byte characters; the ASCII edge rows."""
    rows = [("ab" + chr(cp) + "ab").encode() for _, cp in combinations(table).values()]
    for f in FRAGMENTS:
        rows += [f.encode(), ("the heap " + f + " overflow, " + f + ".").encode(), ("ab" + f + "ab " + f + f).encode()]
    for c in ("\u00df", "\u00e9", "\u20ac", "\u2192", "\U0001f600", "\u4e2d", "\uac00"):
        rows += [(c * k).encode() for k in (99, 100, 101)] + [("q" * 50 + c * 50).encode(), ("q" * 50 + c * 51).encode(), (c * 100 + " " + c).encode()]
    rows += ["caf\u00e9 cafe CAF\u00c9 Caf\u00e9", "ab\u4e2dab \u4e2dab ab\u4e2d", "\uac00\ub098 \ud55c \u1100 \u1161 \uac00\uac00", "\u0130 i\u0307 I \u0131",
             "a\u200bb\u200cc\u200dd\ufeffe\u00adf", "\u200b", " \u00a0\u3000 ", "\u00e9" * 3000, "\u00df " * 3000, "\u4e2d" * 700, "\uac00" * 64]
    rows = [r if isinstance(r, bytes) else r.encode() for r in rows]
    return rows + kit.edge_rows(cased)


def truncation_rows(max_length, add_special=True):
    """The old kit's truncation rows (without its literal row: status rows are tested apart) and rows whose cut falls inside a multi-piece non-ASCII word."""
    budget = max_length - (2 if add_special else 0)
    rows = [r for r in kit.truncation_rows(max_length, add_special) if b"[SEP]" not in r]
    for d in (0, 1, 2, 3):
        lead = " ".join(["ab"] * max(0, budget - d))
        rows += [(lead + " straße heap").encode(), (lead + " 가 heap").encode(), (lead + " a→b€ß").encode(), (lead + "中文").encode()]
    return rows


MALFORMED = [b"ab\x80", b"\x80", b"ab\xbf ab", b"ab\xc3", b"ab\xe4\xb8", b"ab\xf0\x9f\x98", b"\xc3 ab", b"\xe4\xb8 ab", b"\xc3\xc3\xa9", b"\xc0\xaf", b"\xc1\xbf",
             b"\xe0\x80\xaf", b"\xe0\x9f\xbf", b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"ab\xed\xa0\xbd\xed\xb8\x80",
             b"\xf8\x88\x80\x80\x80", b"\xfc\x84\x80\x80\x80\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\xfe", b"\xc3\xa9\xa9", b"a" * 700 + b"\xc3",
             b"caf\xc3\xa9 " * 100 + b"\xa9", "é".encode() * 40 + b"\xe4\xb8"]


def uncovered_examples(rule):
    """{reason: code point} for the reasons of the coverage rule that occur below U+20000 under this tokenizer."""
    found = {}
    for cp in list(range(0x80, 0x3100)) + list(range(0x1D100, 0x1D200)) + list(range(0xFB00, 0xFE00)):
        entry, why = naive_entry(rule.bt, cp)
        if entry is None and why not in found:
            found[why] = cp
    return found


def status_rows(rule):
    """(rows, statuses the premises say they have): every malformed form, U+20000 and beyond, one uncovered code point of each reason that exists, literals
    beside malformed bytes and beside non-ASCII characters."""
    rows = list(MALFORMED)
    want = [2] * len(rows)
    rows += ["𠀀".encode(), "ab𠀀ab".encode(), chr(0x2FFFF).encode(), chr(0x10FFFF).encode(), chr(0xE0001).encode()]
    want += [2] * 5
    for why, cp in sorted(uncovered_examples(rule).items()):
        rows += [chr(cp).encode(), ("heap " + chr(cp) + " heap").encode()]
        want += [2, 2]
    rows += [b"[SEP] \x80", b"\x80[SEP]", b"\xc3[MASK]", "é[MASK]".encode(), "[MASK]é".encode(), "see 𠀀 [CLS]".encode(), "é" .encode() * 400 + b"[PAD]", b"see [SEP] here"]
    want += [1] * 8
    rows += ["é[MASK".encode(), "[sep]é".encode(), "é".encode(), b"plain", b""]
    want += [0] * 5
    return rows, want


# ---- fuzz -------------------------------------------------------------------------------------------------------------------------------------------------------------

def _pool(rule, rng, n=4000):
    cps = [int(c) for c in rng.integers(0x80, 0x20000, size=n) if rule.covered(int(c))]
    cps += [ord(c) for f in FRAGMENTS for c in f if ord(c) >= 0x80 and rule.covered(ord(c))]
    return cps


def _texts(rule, seed, n, stray, ascii_share):
    """n texts of 0 .. 3000 bytes: ASCII dictionary words (``ascii_share`` of the parts) and runs of 1 .. 3 covered code points, glued or spaced; ``stray``: the
    share of the non-ASCII characters that is drawn from all of U+0080 .. U+2FFFF (surrogates apart) instead — about half of those are uncovered, so with
    0.03 and some twenty non-ASCII characters a row (ascii_share 0.93 of ~150 parts) a quarter of the rows holds one."""
    rng = np.random.default_rng(seed)
    words, pool = kit.big_vocab_list()[1], _pool(rule, rng)
    out = []
    for size in rng.integers(0, 3001, size=n):
        parts, have = [], 0
        while have < size:
            r = rng.random()
            if r < ascii_share:
                w = words[int(rng.integers(0, len(words)))]
            else:
                cs = []
                for _ in range(int(rng.integers(1, 4))):
                    cp = pool[int(rng.integers(0, len(pool)))]
                    if stray and rng.random() < stray:
                        cp = int(rng.integers(0x80, 0x30000))
                        cp = cp if not 0xD800 <= cp <= 0xDFFF else 0x20000
                    cs.append(chr(cp))
                w = "".join(cs)
            w += " " if rng.random() < 0.75 else ""
            parts.append(w)
            have += len(w.encode())
        text = "".join(parts).encode()[:int(size)]
        out.append(text.decode("utf-8", "ignore").encode())  # (the cut may fall inside a character: drop the broken tail)
    return tuple(out)


@functools.lru_cache(None)
def _fuzz(cased, seed, stray, ascii_share):
    hf = kit.hf_tokenizer(vocab_list("cased" if cased else "small"), cased)
    return _texts(Rule(hf), seed, 2000, stray, ascii_share)


def fuzz_covered(cased=False):
    """2 000 texts of ASCII words and covered code points only (covered under the normalizer of the cased / uncased tokenizer)."""
    return _fuzz(bool(cased), 20260, 0.0, 0.7)


def fuzz_stray(cased=False):
    """2 000 more, 3 % of their non-ASCII characters arbitrary code points of U+0080 .. U+2FFFF."""
    return _fuzz(bool(cased), 20261, 0.03, 0.93)
