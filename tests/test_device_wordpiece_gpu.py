"""The device WordPiece tokenizer on the GPU (include/memvul_hip.h mv_tok_encode, memvul_amd/csrc/wordpiece.h wp_encode_kernel): byte-equal to
``backend_tokenizer.encode_batch`` of the installed ``tokenizers`` AND to the host restatement on the edge table and both fuzz sets, the launch shapes,
independence of the batching, the drivers end to end with the switch either way, and the tokenising thread next to a resident sweep."""
import json
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plumbing_util as pu  # noqa: E402
import wordpiece_kit as kit  # noqa: E402

pytestmark = pytest.mark.gpu


def _rig(name):
    cased = name == "cased"
    toks = kit.big_vocab_list()[0] if name == "big" else kit.small_vocab_list(cased)
    hf = kit.hf_tokenizer(toks, cased)
    dwp, lits = kit.device_wordpiece(hf, device=0)
    return name, hf, dwp, lits


@pytest.fixture(scope="module", params=["small", "big"])
def rig(request):
    r = _rig(request.param)
    yield r
    r[2].close()


@pytest.fixture(scope="module", params=["small", "big", "cased"])
def edge_rig(request):
    """The rigs of the edge table: the cased one (normalizer lowercase: false) is the only one that runs the kernel without lower-casing."""
    r = _rig(request.param)
    yield r
    r[2].close()


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("add_special", [True, False])
@pytest.mark.parametrize("max_length", kit.MAX_LENGTHS)
def test_edge_table_equals_the_rust_tokenizer_and_the_host_restatement(edge_rig, max_length, add_special):
    name, hf, dwp, lits = edge_rig
    rows = kit.edge_rows(name == "cased") + kit.truncation_rows(max_length, add_special) + [b"see [SEP] here", b"see[MASK]here", b"[sep]", b"[CLS", b"[unused5]", b"ab\x80", b"[PAD]"]
    got = kit.check(dwp.encode, hf, rows, max_length, add_special, lits, name)
    assert _same(got, dwp.encode_host(*kit.pack(rows), max_length, add_special))  # ids with their zero padding, lens, status bytes
    if name == "cased":  # the premise: this tokenizer tells "Buffer" from "buffer" — a kernel that always lower-cased would not pass above
        ids, _ = kit.reference(hf, [b"Buffer", b"buffer", b"HEAP", b"heap"], 8)
        assert ids[0, 1] != ids[1, 1] and ids[2, 1] != ids[3, 1] and hf.unk_token_id not in ids[:, 1].tolist()


@pytest.mark.parametrize("which", ["bytes", "corpus"])
def test_fuzz_equals_the_rust_tokenizer_and_the_host_restatement(rig, which):
    name, hf, dwp, lits = rig
    texts = list(kit.fuzz_bytes() if which == "bytes" else kit.fuzz_corpus())
    got = kit.check(dwp.encode, hf, texts, 256, True, lits, name + " " + which)
    assert not got[2].any() and _same(got, dwp.encode_host(*kit.pack(texts), 256, True))


def test_launch_shapes(rig):
    name, hf, dwp, lits = rig
    pool = list(kit.fuzz_corpus()[:300])
    for n in (257, 1, 3, 4, 5, 255):  # (the largest first, then smaller ones in the grown buffers; four texts to a workgroup)
        kit.check(dwp.encode, hf, pool[:n], 64, True, lits, "%s n=%d" % (name, n))
    ids, lens, status = kit.check(dwp.encode, hf, [b""] * 9, 16, True, lits, name + " all empty")
    assert lens.tolist() == [2] * 9 and not ids[:, 2:].any()
    ids, lens, status = dwp.encode(b"", np.zeros(1, np.int64), 16, True)
    assert ids.shape == (0, 16) and lens.shape == (0,)
    big = (b"overflow heap. " * (3 * (1 << 20) // 15 + 1))[:3 << 20]
    kit.check(dwp.encode, hf, pool[:5] + [big] + pool[5:9] + [b" " * (3 << 20) + b"heap"], 256, True, lits, name + " 3 MiB row")


def test_buffers_grow_across_calls_and_results_do_not_depend_on_the_batching(rig):
    name, hf, dwp, lits = rig
    from memvul_amd.binding import DeviceWordPiece

    texts = list(kit.fuzz_bytes())
    fresh, _ = kit.device_wordpiece(hf, device=0)  # its first call is small, its second larger: every buffer grows
    small = fresh.encode(*kit.pack(texts[:3]), 32, True)
    whole = fresh.encode(*kit.pack(texts), 256, True)
    again = fresh.encode(*kit.pack(texts[:3]), 32, True)
    fresh.close()
    assert _same(small, again) and _same(whole, dwp.encode(*kit.pack(texts), 256, True))
    parts = [dwp.encode(*kit.pack(texts[i:i + 7]), 256, True) for i in range(0, len(texts), 7)]
    assert _same(whole, [np.concatenate([p[k] for p in parts]) for k in range(3)])
    assert isinstance(dwp, DeviceWordPiece)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_with_vocabulary():
    """The plumbing fixture over the 30 522-entry WordPiece vocabulary, a few non-ASCII reports and one that carries [MASK] in its input."""
    fx = pu.make_fixture(n_irs=45, n_anchors=6, layers=2)
    root, arch, golden, test_path = fx[:4]
    vocab = os.path.join(root, "vocab.txt")
    open(vocab, "w", encoding="utf-8").write("\n".join(kit.big_vocab_list()[0]) + "\n")
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


def test_reader_arrays_are_equal_with_the_device_attached(fixture_with_vocabulary):
    from memvul_amd.archive import load_archive

    root, arch, golden, test_path = fixture_with_vocabulary[:4]
    archive = load_archive(arch, cuda_device=0, overrides=pu.TEST_CONFIG, engine_options=EO)
    reader = archive.dataset_reader
    plain = reader.read_arrays(test_path)
    plain_chunks = list(reader.iter_arrays(test_path, chunk=16))
    reader._tokenizer.attach_device(0)
    dev = reader.read_arrays(test_path)
    dev_chunks = list(reader.iter_arrays(test_path, chunk=16))
    counts = dict(reader._tokenizer.device_counts)
    reader._tokenizer.detach_device()
    archive.model.engine.close()
    assert counts == {"device": 2 * (45 - 4), "literal": 2, "non_ascii": 6}
    for a, b in [(plain, dev)] + list(zip(plain_chunks, dev_chunks)):
        assert a["ids"].shape == b["ids"].shape and a["ids"].tobytes() == b["ids"].tobytes() and a["lens"].tobytes() == b["lens"].tobytes()
        assert a["urls"] == b["urls"] and a["labels"] == b["labels"] and a["first"] == b["first"]
    assert len(plain_chunks) == len(dev_chunks) > 2 and plain["lens"].max() > 20


@pytest.mark.parametrize("sweep", ["arrays", False])
def test_drivers_write_identical_files_with_the_switch_either_way(fixture_with_vocabulary, sweep):
    from memvul_amd import predict_memory

    root, arch, golden, test_path = fixture_with_vocabulary[:4]
    out = {}
    for mode in ("host", "gpu"):
        metric = os.path.join(root, "test_results", "tok_%s_%s_metric.json" % (mode, sweep))
        result = os.path.join(root, "test_results", "tok_%s_%s_result.json" % (mode, sweep))
        predict_memory.test_siamese(archive_file=arch, input_file=test_path, input_golden_file=golden, test_config=pu.TEST_CONFIG, output_file=metric,
                                    predictions_output_file=result, batch_size=16, cuda_device=0, engine_options=dict(EO, tokenize=mode), sweep=sweep)
        out[mode] = (open(metric, "rb").read(), open(result, "rb").read())
    assert out["host"][1] == out["gpu"][1] and out["host"][0] == out["gpu"][0]
    assert len(out["gpu"][1]) > 1000 and sum(len(json.loads(l)) for l in out["gpu"][1].decode().splitlines()) == 45


def test_tokenising_thread_next_to_a_resident_sweep(rig):
    """As the array driver uses them: one thread encodes chunks on the tokenizer object while the main thread sweeps a resident corpus on an Engine of the same
    device.  Both results equal their single-threaded ones."""
    import gpu_util
    from memvul_amd import synth

    name, hf, dwp, lits = rig
    eng = gpu_util.engine_for(dict(layers=2, vocab_size=2048), dict(qk_scale=3.0), max_tokens=16384, max_batch=64, max_anchors=64)
    aids, alens = synth.make_ids(5, 64, 2048, seed=synth.SEED + 1, ragged=True, min_len=8)
    ids, lens = synth.make_ids(256, 128, 2048, ragged=True, min_len=4)
    eng.anchor_reset()
    eng.anchor_append(aids, alens)
    alone = eng.bucketed_sweep(ids, lens, 64, with_probs=True)
    texts = list(kit.fuzz_corpus()[:600])
    chunks = [kit.pack(texts[i:i + 100]) for i in range(0, 600, 100)]
    alone_tok = [dwp.encode(p, o, 256, True) for p, o in chunks]
    got_tok, errors = [], []

    def tokenise():
        try:
            for _ in range(3):
                got_tok[:] = [dwp.encode(p, o, 256, True) for p, o in chunks]
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    th = threading.Thread(target=tokenise)
    th.start()
    beside = [eng.bucketed_sweep(ids, lens, 64, with_probs=True) for _ in range(3)]
    th.join()
    assert not errors, errors
    assert len(got_tok) == len(alone_tok) and all(_same(a, b) for a, b in zip(got_tok, alone_tok))
    for b in beside:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b, alone))
