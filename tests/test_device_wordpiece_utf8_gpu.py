"""The UTF-8 mode of the device WordPiece tokenizer on the GPU (include/memvul_hip.h mv_tok_encode_u8, memvul_amd/csrc/wordpiece.h wp_encode_u8_kernel):
byte-equal to ``backend_tokenizer.encode_batch`` of the installed ``tokenizers`` AND to the host restatement (mv_tok_encode_u8_host) — ids with their padding,
lens, status — on the edge and status tables and both fuzz sets, with sequences that straddle the kernel's 64-byte steps, the largest expansion per step,
long carried words, the launch shapes, independence of the batching, and the drivers end to end with the switch at "host" and at "gpu-utf8"."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plumbing_util as pu  # noqa: E402
import wordpiece_kit as kit  # noqa: E402
import wordpiece_utf8_kit as u8  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["small", "big", "cased"])
def rig(request):
    """(name, BertTokenizerFast, DeviceWordPiece on device 0 with the table, the Python rule, the table, cased)."""
    cased = request.param == "cased"
    hf = kit.hf_tokenizer(u8.vocab_list(request.param), cased)
    dwp, lits, table = u8.device_wordpiece(hf, device=0)
    yield request.param, hf, dwp, u8.Rule(hf, lits), table, cased
    dwp.close()


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check(rig, rows, max_length=256, add_special=True, what=""):
    """The kernel against the Rust tokenizer and the Python rule (u8.check) and against the host restatement, byte for byte."""
    name, hf, dwp, rule, table, cased = rig
    got = u8.check(dwp.encode_u8, hf, rule, rows, max_length, add_special, "%s %s" % (name, what))
    assert _same(got, dwp.encode_u8_host(*kit.pack(rows), max_length, add_special)), (name, what)
    return got


@pytest.mark.parametrize("max_length,add_special", [(256, True), (256, False), (2, True), (3, True), (8, True), (8, False), (512, True)])
def test_edge_table_equals_the_rust_tokenizer_and_the_host_restatement(rig, max_length, add_special):
    name, hf, dwp, rule, table, cased = rig
    rows = u8.edge_rows(table, cased) + u8.truncation_rows(max_length, add_special)
    ids, lens, status = _check(rig, rows, max_length, add_special, "edge")
    assert dwp.kernel_ms() > 0  # mv_tok_kernel_ms covers the kernel that ran last
    ascii_rows = [i for i, r in enumerate(rows) if r.isascii()]
    old = dwp.encode(*kit.pack([rows[i] for i in ascii_rows]), max_length, add_special)  # the ASCII kernel on the ASCII rows: the same ids
    assert _same((ids[ascii_rows], lens[ascii_rows], status[ascii_rows]), old) and not status[ascii_rows].any()


def test_status_rows(rig):
    name, hf, dwp, rule, table, cased = rig
    rows, want = u8.status_rows(rule)
    ids, lens, status = _check(rig, rows, 256, True, "status")
    assert status.tolist() == want and not lens[status != 0].any() and not ids[status != 0].any()
    assert dwp.encode(*kit.pack([b"ab\x80", "é".encode(), b"ab"]), 16)[2].tolist() == [1, 1, 0]  # mv_tok_encode on an object with a table: as before


def test_added_tokens_with_bytes_above_0x7f_and_a_hand_marked_table():
    """The kernel's literal test on bytes >= 0x80 (a tokenizer with non-ASCII added tokens: status 1 on the raw bytes, also in the second step of a row and
    across a step's end), and an entry whose covered flag was cleared by hand (status 2)."""
    hf = u8.hf_with_added_tokens()
    dwp, lits, table = u8.device_wordpiece(hf, device=0)
    rule = u8.Rule(hf, lits)
    rows, want = u8.added_token_rows()
    straddle = [("heap " * 30)[:at] + t for at in (61, 62, 63, 64, 125, 127) for t in u8.ADDED]
    rows = rows + [r.encode() for r in straddle]
    want = want + [1] * len(straddle)
    got = u8.check(dwp.encode_u8, hf, rule, rows + list(u8.fuzz_covered()[:200]), 256, True, "added tokens")
    assert got[2][:len(rows)].tolist() == want and _same(got, dwp.encode_u8_host(*kit.pack(rows + list(u8.fuzz_covered()[:200])), 256, True))
    kit.check(dwp.encode, hf, rows + kit.edge_rows()[:140], 256, True, lits, "added tokens, the ASCII kernel")
    edited = table.copy()
    edited["covered"][0xDF] = 0
    dwp.set_unicode(edited)
    sample = ["stra\u00dfe".encode(), "caf\u00e9".encode(), b"heap", ("heap " * 40 + "\u00df").encode()]
    got = dwp.encode_u8(*kit.pack(sample), 16)
    assert got[2].tolist() == [2, 0, 0, 2] and _same(got, dwp.encode_u8_host(*kit.pack(sample), 16))
    dwp.close()


@pytest.mark.parametrize("which", ["covered", "stray"])
def test_fuzz_equals_the_rust_tokenizer_and_the_host_restatement(rig, which):
    name, hf, dwp, rule, table, cased = rig
    texts = list(u8.fuzz_covered(cased) if which == "covered" else u8.fuzz_stray(cased))
    status = _check(rig, texts, 256, True, which)[2]
    assert not status.any() if which == "covered" else 0.05 <= (status == 2).mean() <= 0.40


CHARS = {"2 bytes": "ß", "3 bytes": "€", "4 bytes": "\U0001f600"}


def test_sequences_that_straddle_a_step(rig):
    """One raw byte per lane, 64 to a step: the lead byte of a 2-, 3- and 4-byte character at offsets 60 .. 64 of the first and of the second step, inside a
    word and as its last character; and the same sequence cut by the end of the row, which is malformed."""
    rows, cut = [], []
    for c in CHARS.values():
        for step in (0, 1):
            for at in range(60, 65):
                pad = ("heap " * 30)[:64 * step + at - 2]
                pad = pad[:-1] + " " if pad else pad
                assert len(pad) + 2 == 64 * step + at
                rows += [(pad + "ab" + c + "ab heap").encode(), (pad + "ab" + c + " heap").encode(), (pad + "ab" + c).encode(), (pad + "ab" + c * 40 + "ab").encode()]
                cut += [(pad + "ab").encode() + c.encode()[:k] for k in range(1, len(c.encode()))]
    status = _check(rig, rows + cut, 256, True, "straddle")[2]
    assert not status[:len(rows)].any() and (status[len(rows):] == 2).all()


def test_expansion_and_carried_words(rig):
    """The largest output per step (64 bytes of Hangul syllables with a final consonant: 21 lead bytes x 9 bytes of jamo when accents are stripped), over several
    steps, glued and spaced; a 100-character word of 4-byte characters carried over seven steps, then one more character ([UNK]); a 10^5-character non-ASCII
    word; 50 000 CJK characters, each a word of its own."""
    name, hf, dwp, rule, table, cased = rig
    gak, grin = "각", "\U0001f600"
    if not cased:
        assert table["nbytes"][0xAC01] == 9 and table["nbytes"][table["covered"] == 1].max() == 9
    rows = [gak * 21, gak * 33, gak * 34, gak * 400, " ".join([gak * 5] * 100), " ".join([gak * 33] * 20), "ab" + gak * 33 + "ab", (gak + " ") * 300, (gak + "中") * 150,
            grin * 100, grin * 101, "ab " + grin * 100 + " heap", "ab " + grin * 101 + " heap", "q" + grin * 99, "q" + grin * 100, grin * 100 + "," + grin * 101 + ",ab",
            "ß" * 100000, "€" * 100000 + " heap", "中" * 50000, "é" * 100000]
    ids, lens, status = _check(rig, [r.encode() for r in rows], 256, True, "expansion")
    unk = hf.unk_token_id
    assert not status.any() and ids[10, 1] == unk and lens[10] == 3 and ids[16, 1] == unk and lens[16] == 3 and lens[18] == 256
    assert lens[9] == 102 and unk not in ids[9, :102].tolist()
    _check(rig, [r.encode() for r in rows[:16]], 512, False, "expansion, 512")


def test_launch_shapes(rig):
    name, hf, dwp, rule, table, cased = rig
    pool = list(u8.fuzz_covered(cased)[:300])
    for n in (257, 1, 3, 4, 5, 255):  # (the largest first, then smaller ones in the grown buffers; four texts to a workgroup)
        _check(rig, pool[:n], 64, True, "n=%d" % n)
    ids, lens, status = _check(rig, [b""] * 9, 16, True, "all empty")
    assert lens.tolist() == [2] * 9 and not ids[:, 2:].any()
    ids, lens, status = dwp.encode_u8(b"", np.zeros(1, np.int64), 16, True)
    assert ids.shape == (0, 16) and lens.shape == (0,)
    unit = "straße café 中 overflow 각 heap. ".encode()
    big = (unit * (3 * (1 << 20) // len(unit) + 1))[:3 << 20]
    big = big.decode("utf-8", "ignore").encode()
    _check(rig, pool[:5] + [big] + pool[5:9] + [" ".encode() * (3 << 19) + b"heap"], 256, True, "3 MiB row")


def test_buffers_grow_across_calls_and_results_do_not_depend_on_the_batching(rig):
    name, hf, dwp, rule, table, cased = rig
    texts = list(u8.fuzz_stray(cased))
    fresh, _, _ = u8.device_wordpiece(hf, device=0)  # its first call is small, its second larger: every buffer grows
    small = fresh.encode_u8(*kit.pack(texts[:3]), 32, True)
    whole = fresh.encode_u8(*kit.pack(texts), 256, True)
    again = fresh.encode_u8(*kit.pack(texts[:3]), 32, True)
    ascii_between = fresh.encode(*kit.pack(texts[:3]), 32, True)  # the two kernels share the object's buffers
    fresh.close()
    assert _same(small, again) and _same(whole, dwp.encode_u8(*kit.pack(texts), 256, True)) and ascii_between[2].tolist() == [int(not t.isascii()) for t in texts[:3]]
    parts = [dwp.encode_u8(*kit.pack(texts[i:i + 7]), 256, True) for i in range(0, len(texts), 7)]
    assert _same(whole, [np.concatenate([p[k] for p in parts]) for k in range(3)])


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_with_vocabulary():
    """The fixture of tests/test_device_wordpiece_gpu.py, rebuilt: the plumbing fixture over the big WordPiece vocabulary (here with the non-ASCII pieces),
    the same six non-ASCII reports and the one that carries [MASK] in its input."""
    fx = pu.make_fixture(n_irs=45, n_anchors=6, layers=2)
    root, arch, golden, test_path = fx[:4]
    vocab = os.path.join(root, "vocab.txt")
    toks = list(kit.big_vocab_list()[0])
    toks[-1 - len(u8.PIECES):-1] = u8.PIECES  # (the checkpoint's embedding has 30 522 rows: the pieces take the place of entries, they are not added)
    assert len(toks) == len(set(toks)) == 30522
    open(vocab, "w", encoding="utf-8").write("\n".join(toks) + "\n")
    recs = json.load(open(test_path))
    recs[2]["Issue_Body"] += " café naïve 中文"
    recs[11]["Issue_Title"] = "über " + recs[11]["Issue_Title"]
    recs[30]["Issue_Body"] = "☃"
    recs[7]["Issue_Body"] += " the [MASK] token in a report"
    recs[19]["Issue_Body"] = "Heap\x01Overflow;;; " + recs[19]["Issue_Body"].upper()
    json.dump(recs, open(test_path, "w"))
    old = {k: os.environ.get(k) for k in ("MEMVUL_BERT_VOCAB", "MEMVUL_ALLOW_HASH_TOKENIZER", "MEMVUL_TOKENIZE")}
    os.environ["MEMVUL_BERT_VOCAB"] = vocab
    os.environ.pop("MEMVUL_ALLOW_HASH_TOKENIZER", None)
    os.environ.pop("MEMVUL_TOKENIZE", None)
    yield fx
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


EO = dict(max_tokens=16 * 256, max_batch=16, max_anchors=16)


def test_reader_arrays_are_equal_and_the_non_ascii_rows_stay_on_the_device(fixture_with_vocabulary):
    from memvul_amd.archive import load_archive

    root, arch, golden, test_path = fixture_with_vocabulary[:4]
    archive = load_archive(arch, cuda_device=0, overrides=pu.TEST_CONFIG, engine_options=EO)
    reader = archive.dataset_reader
    tok = reader._tokenizer
    plain = reader.read_arrays(test_path)
    tok.attach_device(0)
    ascii_mode = reader.read_arrays(test_path)
    ascii_counts = dict(tok.device_counts)
    tok.attach_device(0, unicode=True)
    tok.device_counts = {"device": 0, "literal": 0, "non_ascii": 0}
    dev = reader.read_arrays(test_path)
    dev_chunks = list(reader.iter_arrays(test_path, chunk=16))
    counts, unicode_rows = dict(tok.device_counts), tok.device_unicode_rows
    tok.detach_device()
    plain_chunks = list(reader.iter_arrays(test_path, chunk=16))
    archive.model.engine.close()
    assert ascii_counts["non_ascii"] == 3  # one pass over the file under "gpu": the three reports with a byte >= 0x80 stay on the host
    assert counts == {"device": 2 * (45 - 1), "literal": 2, "non_ascii": 0} and unicode_rows == 2 * 3  # two passes under "gpu-utf8": only the [MASK] report comes back
    assert counts["non_ascii"] < ascii_counts["non_ascii"] and unicode_rows > 0
    for a, b in [(plain, dev), (plain, ascii_mode)] + list(zip(plain_chunks, dev_chunks)):
        assert a["ids"].shape == b["ids"].shape and a["ids"].tobytes() == b["ids"].tobytes() and a["lens"].tobytes() == b["lens"].tobytes()
        assert a["urls"] == b["urls"] and a["labels"] == b["labels"] and a["first"] == b["first"]
    assert len(plain_chunks) == len(dev_chunks) > 2 and plain["lens"].max() > 20


@pytest.mark.parametrize("sweep", ["arrays", False])
def test_drivers_write_identical_files_with_the_switch_either_way(fixture_with_vocabulary, sweep):
    from memvul_amd import predict_memory

    root, arch, golden, test_path = fixture_with_vocabulary[:4]
    out = {}
    for mode in ("host", "gpu-utf8"):
        metric = os.path.join(root, "test_results", "tok8_%s_%s_metric.json" % (mode, sweep))
        result = os.path.join(root, "test_results", "tok8_%s_%s_result.json" % (mode, sweep))
        predict_memory.test_siamese(archive_file=arch, input_file=test_path, input_golden_file=golden, test_config=pu.TEST_CONFIG, output_file=metric,
                                    predictions_output_file=result, batch_size=16, cuda_device=0, engine_options=dict(EO, tokenize=mode), sweep=sweep)
        out[mode] = (open(metric, "rb").read(), open(result, "rb").read())
    assert out["host"][1] == out["gpu-utf8"][1] and out["host"][0] == out["gpu-utf8"][0]
    assert len(out["host"][1]) > 1000 and sum(len(json.loads(l)) for l in out["host"][1].decode().splitlines()) == 45
