"""Shared case tables for the device WordPiece tests (tests/test_device_wordpiece_cpu.py, tests/test_device_wordpiece_gpu.py): vocabularies, the edge rows,
the two fuzz sets and the comparison against the reference.  THE REFERENCE of every comparison is ``backend_tokenizer.encode_batch`` of the installed
``tokenizers`` with truncation set as ``PretrainedTransformerTokenizer.batch_ids`` sets it — never the code under test."""
import functools
import os
import string
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LONG_WORD = "q" * 100  # in every vocabulary: a word of exactly max_input_chars_per_word characters that WordPiece still looks up
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
PUNCT = "".join(chr(c) for c in list(range(33, 48)) + list(range(58, 65)) + list(range(91, 97)) + list(range(123, 127)))
MAX_LENGTHS = (2, 3, 8, 12, 256, 512)


def small_vocab_list(cased: bool = False):
    """150 entries.  No 'z', no '##z', no '~': words that hold them have an unmatched remainder."""
    letters = string.ascii_lowercase[:-1]
    toks = list(SPECIALS) + list(letters) + list(string.digits) + [c for c in PUNCT if c != "~"] + ["##" + c for c in letters]
    toks += ["ab", "abab", "buffer", "overflow", "over", "heap", "the", "un", "##able", "##ing", "##s", "##flow", "##ab", "##abab", "stack", "null", "##er",
             "##ed", "free", LONG_WORD, "##" + "b" * 99]
    if cased:
        toks += ["Buffer", "HEAP", "##A", "A", "B", "##B", "Ab", "##Ab"]
    toks = list(dict.fromkeys(toks))
    i = 0
    while len(toks) < 150:
        toks.append("w%dx" % i)
        i += 1
    assert len(toks) == 150 and len(set(toks)) == 150
    return toks


@functools.lru_cache(None)
def big_vocab_list():
    """The synthetic 30 522-entry vocabulary of scripts/r06_e2e_dropin.py (bert-base-uncased's layout), its last entry replaced by LONG_WORD; + its word list."""
    import tempfile

    import r06_e2e_dropin as e2e

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vocab.txt")
        words = e2e.make_vocab(path, np.random.default_rng(11))
        toks = open(path, encoding="utf-8").read().split("\n")[:-1]
    toks[-1] = LONG_WORD
    assert len(toks) == 30522 and len(set(toks)) == 30522
    return toks, sorted(words)


def hf_tokenizer(toks, cased: bool = False):
    from transformers import BertTokenizerFast

    hf = BertTokenizerFast(vocab={t: i for i, t in enumerate(toks)}, do_lower_case=not cased)
    assert hf.vocab_size == len(toks)
    return hf


def wrap(hf, max_length=256, add_special=True):
    """A PretrainedTransformerTokenizer around a BertTokenizerFast that is already in memory (its constructor looks for a vocabulary on disk)."""
    from memvul_amd.tokenizer import PretrainedTransformerTokenizer

    t = PretrainedTransformerTokenizer.__new__(PretrainedTransformerTokenizer)
    t.model_name, t._add_special, t._max_length, t.vocab_size, t._hf = "in-memory", add_special, max_length, hf.vocab_size, hf
    t._device = t._device_encode = None
    t.device_counts = {"device": 0, "literal": 0, "non_ascii": 0}
    return t


def device_wordpiece(hf, device=None):
    """binding.DeviceWordPiece for ``hf`` (device=None: the table only, for encode_host) and the added-token literals it was given."""
    from memvul_amd.binding import DeviceWordPiece

    spec = wrap(hf).device_spec()
    return DeviceWordPiece(device=device, **spec), [l.decode() for l in spec["literals"]]


def reference(hf, texts, max_length, add_special=True):
    """ids int32 [n, max_length] zero-padded and lens int32 [n] from the Rust tokenizer; ``texts`` are bytes below 0x80 (decoded as latin-1 = ASCII)."""
    bt = hf.backend_tokenizer
    bt.enable_truncation(max_length=max_length)
    bt.no_padding()
    encs = bt.encode_batch([t.decode("latin-1") for t in texts], add_special_tokens=add_special)
    ids, lens = np.zeros((len(texts), max_length), np.int32), np.zeros(len(texts), np.int32)
    for i, e in enumerate(encs):
        lens[i] = len(e.ids)
        ids[i, :len(e.ids)] = e.ids
    return ids, lens


def pack(texts):
    off = np.zeros(len(texts) + 1, np.int64)
    if len(texts):
        np.cumsum([len(t) for t in texts], out=off[1:])
    return b"".join(texts), off


def literal_rows(texts, literals):
    """The substring rule in Python: True where a row holds an added-token literal or a byte >= 0x80."""
    lit = [l.encode() for l in literals]
    return np.array([any(l in t for l in lit) or any(b >= 0x80 for b in t) for t in texts], bool)


def check(encode, hf, texts, max_length, add_special=True, literals=SPECIALS, what=""):
    """``encode`` (DeviceWordPiece.encode / encode_host) against the reference on ``texts``: the rows the substring rule names come back with status 1, length
    0 and a zero row; every other row is byte-equal, padding included.  Returns what ``encode`` returned."""
    ids, lens, status = encode(*pack(texts), max_length, add_special)
    ours = ~literal_rows(texts, literals)
    assert status.tolist() == (~ours).astype(np.uint8).tolist(), (what, "status", np.flatnonzero(status != (~ours)).tolist()[:5])
    want_ids, want_lens = reference(hf, [t if o else b"" for t, o in zip(texts, ours)], max_length, add_special)
    want_ids[~ours], want_lens[~ours] = 0, 0
    bad = np.flatnonzero((lens != want_lens) | (ids != want_ids).any(1))
    assert not len(bad), (what, max_length, add_special, int(bad[0]), texts[int(bad[0])][:200], ids[bad[0], :16].tolist(), want_ids[bad[0], :16].tolist(),
                          int(lens[bad[0]]), int(want_lens[bad[0]]))
    return ids, lens, status


def edge_rows(cased: bool = False):
    """The edge table (bytes).  The same rows serve every vocabulary; what is a word and what is [UNK] differs, the reference decides."""
    rows = [b"ab" + bytes([c]) + b"ab" for c in range(128)]
    rows += [b"q" * 99, b"q" * 100, b"q" * 101, b"a" * 100 + b"b" * 99, b"a" * 100 + b"b" * 100, b"a" * 100 + b" " + b"b" * 99, b"a" * 99 + b"##b",
             b"q" * 100 + b"b" * 99, b"abz", b"bufferz overflow", b"unablez", b"abab~", b"", b" ", b" \t\n\r  ", PUNCT.encode(), PUNCT.encode() * 3,
             b"Buffer OVERFLOW in HeAp the Stack", b"AbAb aBAB", b" " * (1 << 20) + b"heap", b"a" * 100000, b"ab " * 50000,
             b"the buffer overflows, unable; stacking null-free", b"\x01\x02ab\x7f", b"ab\x00", b"\x0b\x0c", b"ab\x1fab ab\x0bab ab\x0cab", b"a" * 63 + b" " + b"b" * 64,
             b"a" * 64, b"a" * 64 + b" ab", b"ab" * 32 + b"abab", b"x" * 37 + b" " + b"ab" * 45 + b"." + b"q" * 100 + b",heap"]
    if cased:
        rows += [b"Buffer HEAP buffer heap AB Ab aB", b"ABAB AbAb"]
    return rows


def truncation_rows(max_length, add_special=True):
    """Texts of max_length - 3, - 2 and - 1 words "ab" (one token each in the small vocabularies), one of exactly as many as the token budget holds with or
    without the special tokens, one whose cut falls between the pieces of one word, and a full row followed by a literal (a status row)."""
    budget = max_length - (2 if add_special else 0)
    rows = [b" ".join([b"ab"] * max(0, max_length - d)) for d in (3, 2, 1)]
    rows += [b" ".join([b"ab"] * budget), b" ".join([b"ab"] * (budget + 1)), b" ".join([b"ab"] * max(0, budget - 1)) + b" heapabab heap", b" ".join([b"ab"] * max(0, budget)) + b" [SEP]", b"overflows " * max_length]
    return rows


@functools.lru_cache(None)
def fuzz_bytes(n=2000, seed=20250):
    """n texts of 0 .. 3000 random bytes below 0x80, every byte value possible."""
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 128, size=int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 3001, size=n))


@functools.lru_cache(None)
def fuzz_corpus(n=2000, seed=20251):
    """n texts in the style of scripts/r06_e2e_dropin.make_corpus: dictionary words, identifiers that split into pieces, numbers, punctuation."""
    rng = np.random.default_rng(seed)
    words = big_vocab_list()[1]
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz_"))
    idents = ["".join(letters[rng.integers(0, len(letters), size=int(k))]) for k in rng.integers(5, 14, size=512)]
    punct = list(".,:;()[]/-")

    def text(nw):
        r = rng.random(nw)
        wi, ii = rng.integers(0, len(words), size=nw), rng.integers(0, len(idents), size=nw)
        num, pi = rng.integers(0, 100000, size=nw), rng.integers(0, len(punct), size=nw)
        return " ".join(words[wi[j]] if r[j] < 0.8 else idents[ii[j]] if r[j] < 0.92 else str(num[j]) if r[j] < 0.96 else punct[pi[j]] for j in range(nw))

    return tuple(("%s. %s" % (text(int(rng.integers(4, 12))), text(int(rng.integers(8, 200))))).encode() for _ in range(n))
