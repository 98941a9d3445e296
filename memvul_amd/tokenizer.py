"""``pretrained_transformer`` tokenizer / indexer stand-ins (AllenNLP names used by the reference
configs: test_config_memory.json:5-16, config_memory.json:15-27).

Behaviour kept from AllenNLP's ``PretrainedTransformerTokenizer``: lower-cased WordPiece of
``bert-base-uncased`` with ``[CLS] ... [SEP]`` added and truncation to ``max_length`` INCLUDING the two
special tokens (256 for issue reports, 512 for anchors).  The real WordPiece vocabulary is used when a
``vocab.txt`` is reachable (``model_name`` is a directory holding one, or ``$MEMVUL_BERT_VOCAB``); it is
not on disk in this image and there is no network, so otherwise a deterministic hashing word tokenizer
with the same id range / special ids is used — enough for plumbing and throughput runs on synthetic
text, not for real accuracy numbers.
"""
from __future__ import annotations

import logging
import os
import re
import zlib
from typing import Dict, List, Optional

from .data import Token
from .registry import Tokenizer, TokenIndexer, register_builtin

logger = logging.getLogger(__name__)
CLS_ID, SEP_ID, PAD_ID, UNK_ID = 101, 102, 0, 100
_WORD_RE = re.compile(r"[a-z0-9]+|[^\sa-z0-9]")


def _find_vocab(model_name: str) -> Optional[str]:
    cands = [os.environ.get("MEMVUL_BERT_VOCAB")]
    if model_name and os.path.isdir(model_name):
        cands.append(os.path.join(model_name, "vocab.txt"))
    for c in cands:
        if c and os.path.isfile(c):
            return c
    return None


def code_point_table(backend_tokenizer):
    """The code-point table of the device tokenizer's UTF-8 rule (memvul_amd/csrc/wordpiece.h; binding.CODE_POINT_DTYPE [0x20000], entry i for code point i),
    read from the tokenizer itself: the output bytes are ``normalizer.normalize_str(chr(cp))`` — clean, CJK spacing, accent stripping and lower-casing are
    whatever this normalizer does, probed, not assumed — and the class of every output character is what ``pre_tokenizer.pre_tokenize_str("a" + c + "a")``
    shows: ["a", c, "a"] punctuation, ["a", "a"] whitespace, ["a" + c + "a"] a word character.  A code point is left UNCOVERED (a row that holds it is handed
    back, status 2) when Python's unicodedata calls it unassigned (the Rust crate may know a newer Unicode), when its output keeps a character of non-zero
    canonical combining class (NFD reorders those: the normalizer is not context-free there), when the output exceeds 3 code points or 12 bytes, or when an
    output character's probe is none of the three patterns.  Entries below 0x80 stay zero: the ASCII rule never reads them."""
    import unicodedata

    import numpy as np

    from .binding import CODE_POINT_DTYPE, CODE_POINTS

    norm, pre = backend_tokenizer.normalizer, backend_tokenizer.pre_tokenizer
    raw = bytearray(16 * CODE_POINTS)
    classes: Dict[str, int] = {}

    def class_of(c: str) -> int:
        k = classes.get(c)
        if k is None:
            got = [w for w, _ in pre.pre_tokenize_str("a" + c + "a")]
            k = classes[c] = 3 if got == ["a" + c + "a"] else 2 if got == ["a", c, "a"] else 1 if got == ["a", "a"] else 0
        return k

    for cp in range(0x80, CODE_POINTS):
        if 0xD800 <= cp <= 0xDFFF:  # no scalar values: in UTF-8 they are malformed sequences
            continue
        ch = chr(cp)
        if unicodedata.category(ch) == "Cn":
            continue
        out = norm.normalize_str(ch)
        if len(out) > 3 or any(unicodedata.combining(c) for c in out):
            continue
        b = out.encode("utf-8")
        ks = [class_of(c) for c in out]
        if len(b) > 12 or 0 in ks:
            continue
        raw[16 * cp:16 * cp + len(b)] = b
        raw[16 * cp + 12:16 * cp + 16] = bytes((len(b), sum(k << (2 * j) for j, k in enumerate(ks)), 1, len(out)))
    return np.frombuffer(bytes(raw), CODE_POINT_DTYPE)


class TokenRow:
    """The tokens of one text as a sequence over its id array: ``len``, iteration and indexing give ``Token`` objects (built when asked for: with
    the WordPiece backend their ``text`` is looked up then), ``ids`` gives the int32 array the collation reads directly — a file of 40 k issue
    reports is 8 M tokens, and one Python object per token costs more than the tokenisation itself."""

    __slots__ = ("ids", "_hf")

    def __init__(self, ids, hf=None):
        self.ids, self._hf = ids, hf

    def __len__(self):
        return len(self.ids)

    def _tok(self, i: int) -> Token:
        return Token(self._hf.convert_ids_to_tokens(i) if self._hf is not None else str(i), i, 0)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return TokenRow(self.ids[k], self._hf)
        return self._tok(int(self.ids[k]))

    def __iter__(self):
        if self._hf is not None:
            ids = [int(i) for i in self.ids]
            return (Token(t, i, 0) for t, i in zip(self._hf.convert_ids_to_tokens(ids), ids))
        return (Token(str(int(i)), int(i), 0) for i in self.ids)

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all((a.text, a.text_id, a.type_id) == (b.text, b.text_id, b.type_id) for a, b in zip(self, other))
        except (TypeError, AttributeError):
            return NotImplemented


@register_builtin(Tokenizer, "pretrained_transformer")
class PretrainedTransformerTokenizer(Tokenizer):
    def __init__(self, model_name: str = "bert-base-uncased", add_special_tokens: bool = True, max_length: Optional[int] = None,
                 tokenizer_kwargs: Optional[Dict] = None, vocab_size: int = 30522) -> None:
        self.model_name, self._add_special, self._max_length = model_name, add_special_tokens, max_length
        self.vocab_size = vocab_size
        self._hf = None
        self._device = None          # attach_device: the binding.DeviceWordPiece the ASCII rows of batch_ids go through
        self._device_encode = None
        # rows batch_ids tokenised on the device / got back for an added-token literal (status 1) / kept off it for a byte >= 0x80, or with unicode=True got back
        # for a malformed sequence or an uncovered code point (status 2)
        self.device_counts = {"device": 0, "literal": 0, "non_ascii": 0}
        self._device_unicode = False   # attach_device(unicode=True): batch_ids sends every row to the device in UTF-8
        self._code_points = None       # its code-point table, built once per tokenizer object
        self.device_unicode_rows = 0   # rows with a byte >= 0x80 that batch_ids tokenised on the device
        vocab = _find_vocab(model_name)
        if vocab is None:
            # a cached / local HuggingFace copy of `model_name` (what AllenNLP's tokenizer loads, reader_memory.py:88)
            try:
                from transformers import BertTokenizerFast

                hf = BertTokenizerFast.from_pretrained(model_name, local_files_only=True, **(tokenizer_kwargs or {}))
                # transformers 5.x hands back a 5-token default vocabulary instead of raising when nothing is cached
                if hf.vocab_size >= 1000 and hf.cls_token_id is not None and hf.sep_token_id is not None:
                    self._hf = hf
                    self.vocab_size = hf.vocab_size
            except Exception:
                self._hf = None
            if self._hf is None:
                if os.environ.get("MEMVUL_ALLOW_HASH_TOKENIZER") != "1":
                    raise RuntimeError(
                        f"no WordPiece vocabulary for {model_name!r}: point $MEMVUL_BERT_VOCAB at its vocab.txt (or make model_name "
                        "a directory holding one, or have it in the local HuggingFace cache).  The CRC32 hashing stand-in feeds "
                        "meaningless ids to trained weights; it is only for synthetic plumbing / throughput runs and must be "
                        "asked for with MEMVUL_ALLOW_HASH_TOKENIZER=1.")
                logger.warning("MEMVUL_ALLOW_HASH_TOKENIZER=1: %r is tokenised by the CRC32 hashing stand-in (synthetic runs only)", model_name)
        if vocab is not None:
            import inspect

            from transformers import BertTokenizerFast

            with open(vocab, "r", encoding="utf-8") as f:
                table = {line.rstrip("\n"): i for i, line in enumerate(f)}
            # transformers 4.x (the reference pins 4.1.0) takes ``vocab_file``; 5.x takes ``vocab`` and silently IGNORES
            # ``vocab_file`` (a 5-token default vocabulary comes back) — so pick by signature and check the result
            if "vocab" in inspect.signature(BertTokenizerFast.__init__).parameters:
                self._hf = BertTokenizerFast(vocab=table, do_lower_case=True, **(tokenizer_kwargs or {}))
            else:
                self._hf = BertTokenizerFast(vocab_file=vocab, do_lower_case=True, **(tokenizer_kwargs or {}))
            if self._hf.vocab_size != len(table) or self._hf.cls_token_id != table.get("[CLS]") or self._hf.sep_token_id != table.get("[SEP]"):
                raise RuntimeError(f"WordPiece vocabulary {vocab} was not taken over by BertTokenizerFast "
                                   f"({self._hf.vocab_size} tokens loaded, {len(table)} in the file)")
            self.vocab_size = self._hf.vocab_size

    def _hash_ids(self, text: str) -> List[int]:
        lo = 1000 if self.vocab_size > 2000 else 3
        return [lo + zlib.crc32(w.encode("utf-8")) % (self.vocab_size - lo) for w in _WORD_RE.findall(text.lower())]

    def _hash_encode(self, text: str) -> List[int]:
        ids = self._hash_ids(text)
        if self._add_special:
            if self._max_length is not None:
                ids = ids[: max(0, self._max_length - 2)]
            return [CLS_ID] + ids + [SEP_ID]
        return ids[: self._max_length] if self._max_length is not None else ids

    def device_spec(self) -> Dict:
        """What binding.DeviceWordPiece needs, read from the serialised backend tokenizer — or a ValueError naming the field that makes this tokenizer something
        the device rule (memvul_amd/csrc/wordpiece.h) does not restate.  No silent fallback: a tokenizer that is refused stays on the host because the caller
        sees the error."""
        import json

        if self._hf is None or getattr(self._hf, "backend_tokenizer", None) is None:
            raise ValueError("attach_device: the CRC32 hashing stand-in (no WordPiece backend) is not what the device tokenizer restates")
        d = json.loads(self._hf.backend_tokenizer.to_str())
        model, norm, pre, post = d.get("model") or {}, d.get("normalizer") or {}, d.get("pre_tokenizer") or {}, d.get("post_processor") or {}

        def need(where, field, got, want):
            if got != want:
                raise ValueError(f"attach_device: {where}.{field} is {got!r}, the device tokenizer restates {want!r} only")

        need("model", "type", model.get("type"), "WordPiece")
        need("model", "continuing_subword_prefix", model.get("continuing_subword_prefix"), "##")
        need("normalizer", "type", norm.get("type"), "BertNormalizer")
        need("normalizer", "clean_text", norm.get("clean_text"), True)
        need("pre_tokenizer", "type", pre.get("type"), "BertPreTokenizer")
        vocab = model["vocab"]
        if post.get("type") == "TemplateProcessing":
            single = post.get("single") or []
            shape = [next(iter(x)) for x in single]
            if shape != ["SpecialToken", "Sequence", "SpecialToken"]:
                raise ValueError(f"attach_device: post_processor.single is {shape!r}, the device tokenizer restates [CLS] A [SEP] only")
            cls_tok, sep_tok = single[0]["SpecialToken"]["id"], single[2]["SpecialToken"]["id"]
            cls_id, sep_id = post["special_tokens"][cls_tok]["ids"], post["special_tokens"][sep_tok]["ids"]
            if len(cls_id) != 1 or len(sep_id) != 1:
                raise ValueError("attach_device: post_processor.special_tokens: a special token of more than one id")
            cls_id, sep_id = cls_id[0], sep_id[0]
        elif post.get("type") == "BertProcessing":
            cls_id, sep_id = post["cls"][1], post["sep"][1]
        else:
            raise ValueError(f"attach_device: post_processor.type is {post.get('type')!r}, the device tokenizer restates [CLS] A [SEP] only")
        literals = []
        for a in d.get("added_tokens") or []:
            if a.get("normalized"):  # matched AFTER normalisation: a raw substring search does not find what the backend finds
                raise ValueError(f"attach_device: added_tokens[{a.get('content')!r}].normalized is True, the device tokenizer hands back raw literals only")
            if a.get("content"):
                literals.append(a["content"].encode("utf-8"))
        unk = model.get("unk_token")
        if unk not in vocab:
            raise ValueError(f"attach_device: model.unk_token {unk!r} is not in the vocabulary")
        pieces = [b""] * (max(vocab.values()) + 1)
        for tok, i in vocab.items():
            pieces[i] = tok.encode("utf-8")
        return {"vocab": pieces, "literals": literals, "unk_id": vocab[unk], "cls_id": cls_id, "sep_id": sep_id,
                "max_chars_per_word": int(model.get("max_input_chars_per_word", 100)), "lowercase": bool(norm.get("lowercase"))}

    def attach_device(self, device_index: int = 0, host_restatement: bool = False, unicode: bool = False):
        """Tokenise the ASCII rows of ``batch_ids`` on GPU ``device_index`` (binding.DeviceWordPiece); every other row, and every row that comes back for an
        added-token literal, keeps going through the Rust tokenizer: the arrays are those of the host path for every input.  Raises, naming the field, when
        the backend is not what the device rule restates (device_spec) or ``max_length`` is outside 2 .. 512.  ``max_length=None`` attaches but leaves
        batch_ids on the host: without it neither the row width nor the work per row is bounded.  ``host_restatement``: run the same rule through
        mv_tok_encode_host instead, no GPU — for tests; no switch selects it.  ``unicode``: the UTF-8 rule instead — EVERY row goes to the device, packed as
        UTF-8 (mv_tok_encode_u8), with the code-point table built from this tokenizer's own normalizer and pre-tokenizer (code_point_table, once per tokenizer
        object); the rows that come back — an added-token literal, or a malformed sequence / a code point the table does not cover — go through the Rust
        tokenizer as before."""
        from .binding import DeviceWordPiece

        spec = self.device_spec()
        if self._max_length is not None and not 2 <= int(self._max_length) <= 512:
            raise ValueError(f"attach_device: max_length is {self._max_length!r}, the device tokenizer takes 2 .. 512")
        self.detach_device()
        self._device = DeviceWordPiece(device=None if host_restatement else int(device_index), **spec)
        self._device_encode = self._device.encode_host if host_restatement else self._device.encode
        self._device_unicode = bool(unicode)
        if unicode:
            try:
                if self._code_points is None:
                    self._code_points = code_point_table(self._hf.backend_tokenizer)
                self._device.set_unicode(self._code_points)
            except Exception:
                self.detach_device()
                raise
            self._device_encode = self._device.encode_u8_host if host_restatement else self._device.encode_u8
        return self

    def detach_device(self):
        if self._device is not None:
            self._device.close()
        self._device = self._device_encode = None
        self._device_unicode = False

    def _device_batch_ids(self, bt, texts: List[str]):
        """batch_ids with a device attached: ASCII rows packed and encoded there, the rest — and the rows handed back — in ONE encode_batch call, merged in
        the caller's order and trimmed to the longest row, exactly the arrays of the host path."""
        import numpy as np

        n, width = len(texts), int(self._max_length)
        flags = np.fromiter((t.isascii() for t in texts), dtype=bool, count=n)  # (a flag read in CPython)
        asc = np.flatnonzero(flags)
        back = np.zeros(0, np.int64)
        ids, lens = None, np.zeros(n, np.int32)
        if len(asc):
            rows = texts if len(asc) == n else [texts[i] for i in asc]
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum(np.fromiter((len(t) for t in rows), np.int64, len(rows)), out=off[1:])  # (ASCII: characters = bytes)
            d_ids, d_lens, d_status = self._device_encode("".join(rows).encode("ascii"), off, width, self._add_special)
            back = asc[d_status != 0]
            if len(asc) == n:
                ids, lens = d_ids, d_lens
            else:
                ids = np.zeros((n, width), np.int32)
                ids[asc], lens[asc] = d_ids, d_lens
        else:
            ids = np.zeros((n, width), np.int32)
        rest = np.sort(np.concatenate([np.flatnonzero(~flags), back]))
        if len(rest):
            bt.enable_truncation(max_length=self._max_length)
            bt.no_padding()
            for i, e in zip(rest, bt.encode_batch([texts[i] for i in rest], add_special_tokens=self._add_special)):
                lens[i] = len(e)
                ids[i, :len(e)] = e.ids
        self.device_counts["device"] += len(asc) - len(back)
        self.device_counts["literal"] += len(back)
        self.device_counts["non_ascii"] += n - len(asc)
        return np.ascontiguousarray(ids[:, :int(lens.max())]), lens

    def _device_batch_ids_unicode(self, bt, texts: List[str]):
        """batch_ids with a device attached with unicode=True: all rows packed as UTF-8 (a lone surrogate passes as the malformed sequence it is and comes
        back) and encoded there in ONE call; the rows handed back in ONE encode_batch call, as above."""
        import numpy as np

        n, width = len(texts), int(self._max_length)
        flags = np.fromiter((t.isascii() for t in texts), dtype=bool, count=n)
        nbytes = np.fromiter((len(t) for t in texts), np.int64, n)  # (characters = bytes for the ASCII rows; the others are counted below)
        for i in np.flatnonzero(~flags):
            nbytes[i] = len(texts[i].encode("utf-8", "surrogatepass"))
        off = np.zeros(n + 1, np.int64)
        np.cumsum(nbytes, out=off[1:])
        ids, lens, status = self._device_encode("".join(texts).encode("utf-8", "surrogatepass"), off, width, self._add_special)
        back = np.flatnonzero(status != 0)
        if len(back):
            bt.enable_truncation(max_length=self._max_length)
            bt.no_padding()
            for i, e in zip(back, bt.encode_batch([texts[i] for i in back], add_special_tokens=self._add_special)):
                lens[i] = len(e)
                ids[i, :len(e)] = e.ids
        self.device_counts["device"] += n - len(back)
        self.device_counts["literal"] += int((status == 1).sum())
        self.device_counts["non_ascii"] += int((status == 2).sum())
        self.device_unicode_rows += int((~flags & (status == 0)).sum())
        return np.ascontiguousarray(ids[:, :int(lens.max())]), lens

    def batch_ids(self, texts: List[str], workers: int = 0):
        """Array form of ``tokenize`` for a whole file: ``(ids int32 [N, L] zero-padded, lens int32 [N])`` with exactly the
        ids ``tokenize`` gives text by text.  The WordPiece path is one batched call into the Rust tokenizer (parallel
        inside); the hashing stand-in can fan out over ``workers`` forked processes."""
        import numpy as np

        bt = getattr(self._hf, "backend_tokenizer", None) if self._hf is not None else None
        if bt is not None and len(texts) and self._device_encode is not None and self._max_length is not None:
            return (self._device_batch_ids_unicode if self._device_unicode else self._device_batch_ids)(bt, list(texts))
        if bt is not None and len(texts):
            # the Rust tokenizer itself, not the transformers wrapper around it: the wrapper turns every encoding into dicts of Python lists under the interpreter
            # lock (1.3 s of a 1.8 s call for 8 k reports; the same ids: tests/test_plumbing.py) — here the ids go from the encodings into ONE flat int32 array and from
            # there into the padded matrix, no Python object per token or per text
            import itertools

            if self._max_length is not None:
                bt.enable_truncation(max_length=self._max_length)  # (longest_first, right, stride 0: what truncation=True asks of the wrapper)
            else:
                bt.no_truncation()
            bt.no_padding()
            encs = bt.encode_batch(list(texts), add_special_tokens=self._add_special)
            lens = np.fromiter((len(e) for e in encs), dtype=np.int32, count=len(encs))
            flat = np.fromiter(itertools.chain.from_iterable(e.ids for e in encs), dtype=np.int32, count=int(lens.sum()))
            L = int(lens.max())
            ids = np.zeros((len(encs), L), np.int32)
            ids[np.arange(L)[None, :] < lens[:, None]] = flat
            return ids, lens
        if self._hf is not None:
            rows = self._hf(list(texts), add_special_tokens=self._add_special, truncation=self._max_length is not None,
                            max_length=self._max_length, return_attention_mask=False, return_token_type_ids=False)["input_ids"]
        elif workers and workers > 1 and len(texts) >= 4 * workers:
            import multiprocessing as mp

            step = (len(texts) + workers - 1) // workers
            with mp.get_context("fork").Pool(workers) as pool:
                parts = pool.map(self._hash_encode_many, [texts[i:i + step] for i in range(0, len(texts), step)])
            rows = [r for part in parts for r in part]
        else:
            rows = self._hash_encode_many(texts)
        lens = np.fromiter((len(r) for r in rows), dtype=np.int32, count=len(rows))
        ids = np.zeros((len(rows), int(lens.max()) if len(rows) else 0), np.int32)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        return ids, lens

    def _hash_encode_many(self, texts: List[str]) -> List[List[int]]:
        return [self._hash_encode(t) for t in texts]

    def batch_token_rows(self, texts: List[str]) -> List["TokenRow"]:
        """``batch_tokenize`` without the Token objects: one TokenRow per text (same tokens, same ids, materialised on demand)."""
        ids, lens = self.batch_ids(texts)
        return [TokenRow(ids[i, :lens[i]], self._hf) for i in range(len(texts))]

    def batch_tokenize(self, texts: List[str]) -> List[List[Token]]:
        """``[tokenize(t) for t in texts]`` with ONE call into the tokenizer backend (same tokens, same ids)."""
        ids, lens = self.batch_ids(texts)
        rows = [ids[i, :lens[i]].tolist() for i in range(len(texts))]
        if self._hf is not None:
            return [[Token(t, i, 0) for t, i in zip(self._hf.convert_ids_to_tokens(r), r)] for r in rows]
        return [[Token(str(i), i, 0) for i in r] for r in rows]

    def tokenize(self, text: str) -> List[Token]:
        if self._hf is not None:
            enc = self._hf(text, add_special_tokens=self._add_special, truncation=self._max_length is not None,
                           max_length=self._max_length, return_attention_mask=False, return_token_type_ids=False)
            ids = enc["input_ids"]
            texts = self._hf.convert_ids_to_tokens(ids)
            return [Token(t, i, 0) for t, i in zip(texts, ids)]
        return [Token(str(i), i, 0) for i in self._hash_encode(text)]


@register_builtin(TokenIndexer, "pretrained_transformer")
class PretrainedTransformerIndexer(TokenIndexer):
    """Tokens already carry their wordpiece ids; indexing is the identity (``namespace`` is only where
    AllenNLP would mirror the HF vocabulary)."""

    def __init__(self, model_name: str = "bert-base-uncased", namespace: str = "tags", max_length: Optional[int] = None, **_kw) -> None:
        self.model_name, self._namespace, self._max_length = model_name, namespace, max_length

    def tokens_to_indices(self, tokens: List[Token], vocabulary=None) -> Dict[str, List]:
        return {"token_ids": [t.text_id for t in tokens], "mask": [True] * len(tokens), "type_ids": [t.type_id or 0 for t in tokens]}
