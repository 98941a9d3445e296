"""What the device WordPiece tokenizer (MEMVUL_TOKENIZE=gpu) buys, measured: ``batch_ids`` on the host and through the device, and the whole job either way.
The 40 k-report corpus and the synthetic 30 522-entry vocabulary of scripts/r06_e2e_dropin.py; three alternating repeats of everything.

  batch_ids texts/s, 16 384-text chunks: host (the threads the box gives), host with RAYON_NUM_THREADS=2 (what one of eight ranks gets; a child process of its own:
      the Rust thread pool is sized once), device (pack + mv_tok_encode + merge, as the drivers call it)
  mv_tok_encode alone per chunk (upload + kernel + download: the call is synchronous) and the kernel's own time in it (HIP events around the launch,
      mv_tok_kernel_ms)
  test_siamese(sweep="arrays") whole-job issue reports/s with the switch either way

WHAT IT IS HELD TO (printed as PASS / FAIL with the spreads): the device path's batch_ids rate exceeds the host path's on the same box by more than the
repeat-to-repeat spread of the two; the whole-job rate with gpu is not lower than with host by more than that spread.  The ratio at two threads is reported.
Usage (GPU box): python scripts/gpu_tokenizer_rate.py [N] > profiles/gpu_tokenizer_bench.txt"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

CHUNK = 16384


def texts_of(test_path):
    recs = json.load(open(test_path))
    return ["%s. %s" % (r["Issue_Title"], r["Issue_Body"]) for r in recs]


def tokenizer():
    from memvul_amd.tokenizer import PretrainedTransformerTokenizer

    return PretrainedTransformerTokenizer("bert-base-uncased", max_length=256)  # ($MEMVUL_BERT_VOCAB names the vocabulary)


def rate(tok, texts):
    t0 = time.perf_counter()
    for i in range(0, len(texts), CHUNK):
        tok.batch_ids(texts[i:i + CHUNK])
    return len(texts) / (time.perf_counter() - t0)


def child_host(test_path):
    texts, tok = texts_of(test_path), tokenizer()
    rate(tok, texts[:2048])
    print(json.dumps([rate(tok, texts) for _ in range(3)]))


def spread(*lists):
    return max(max(l) - min(l) for l in lists)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    import plumbing_util as pu
    import r06_e2e_dropin as e2e
    from memvul_amd import predict_memory as pm

    rng = np.random.default_rng(11)
    root, arch, _, _, w, dims = pu.make_fixture(n_irs=4, n_anchors=4, layers=12)
    vocab = os.path.join(root, "vocab.txt")
    words = e2e.make_vocab(vocab, rng)
    os.environ["MEMVUL_BERT_VOCAB"] = vocab
    os.environ.pop("MEMVUL_ALLOW_HASH_TOKENIZER", None)
    os.environ.pop("MEMVUL_TOKENIZE", None)
    golden, test_path = e2e.make_corpus(root, rng, words, n)
    texts = texts_of(test_path)
    print("N = %d issue reports (%.1f MB of text), chunks of %d, max_length 256, host cores %d, tokenizers' thread pool: the box's default"
          % (n, sum(map(len, texts)) / 1e6, CHUNK, os.cpu_count()), flush=True)

    host, dev = tokenizer(), tokenizer().attach_device(0)
    a, b = host.batch_ids(texts[:4096]), dev.batch_ids(texts[:4096])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    r_host, r_dev = [], []
    for _ in range(3):
        r_host.append(rate(host, texts))
        r_dev.append(rate(dev, texts))
    env = dict(os.environ, RAYON_NUM_THREADS="2")
    r_host2 = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--child-host", test_path], env=env, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    print("batch_ids, texts/s, three repeats each (host and device alternating):")
    print("  host, default threads     %s" % "  ".join("%8.0f" % r for r in r_host))
    print("  host, RAYON_NUM_THREADS=2 %s" % "  ".join("%8.0f" % r for r in r_host2))
    print("  device                    %s   rows: %s" % ("  ".join("%8.0f" % r for r in r_dev), dev.device_counts))
    s1 = spread(r_host, r_dev)
    ok1 = min(r_dev) - max(r_host) > 0 and np.mean(r_dev) - np.mean(r_host) > s1
    print("  device / host = %.2f (means); device / host at two threads = %.2f (reported, not bounded); repeat-to-repeat spread %.0f texts/s"
          % (np.mean(r_dev) / np.mean(r_host), np.mean(r_dev) / np.mean(r_host2), s1))
    print("  STATEMENT 1 — the device path's batch_ids rate exceeds the host path's by more than that spread: %s" % ("PASS" if ok1 else "FAIL"), flush=True)

    packed = []
    for i in range(0, len(texts), CHUNK):
        rows = texts[i:i + CHUNK]
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(t) for t in rows], out=off[1:])
        packed.append(("".join(rows).encode("ascii"), off))
    per_chunk = []
    for _ in range(3):
        for p, o in packed:
            t0 = time.perf_counter()
            dev._device.encode(p, o, 256, True)
            per_chunk.append((time.perf_counter() - t0, len(o) - 1, len(p), dev._device.kernel_ms()))
    full = [t for t, m, _, _ in per_chunk if m == CHUNK]
    kern = [k for _, m, _, k in per_chunk if m == CHUNK]
    print("mv_tok_encode alone (upload + kernel + download, synchronous), %d-text chunks of %.1f MB: min %.1f ms, median %.1f ms, max %.1f ms = %.0f texts/s at the median"
          % (CHUNK, np.mean([b for _, m, b, _ in per_chunk if m == CHUNK]) / 1e6, min(full) * 1e3, np.median(full) * 1e3, max(full) * 1e3, CHUNK / np.median(full)), flush=True)
    print("  the tokenise kernel's own time in it (HIP events): min %.2f ms, median %.2f ms, max %.2f ms per chunk = %.0f texts/s at the median"
          % (min(kern), np.median(kern), max(kern), CHUNK / (np.median(kern) / 1e3)), flush=True)
    dev.detach_device()

    eo = dict(max_tokens=512 * 256, max_batch=512, max_anchors=128)
    out = os.path.join(root, "test_results", "pred.json")
    jobs = {"host": [], "gpu": []}
    files = {}
    for rep in range(3):
        for mode in ("host", "gpu"):
            t0 = time.perf_counter()
            archive_s = [0.0]
            load = pm.load_archive

            def timed_load(*a, **k):
                t = time.perf_counter()
                try:
                    return load(*a, **k)
                finally:
                    archive_s[0] += time.perf_counter() - t
            pm.load_archive = timed_load
            try:
                pm.test_siamese(arch, test_path, golden, test_config=pu.TEST_CONFIG, predictions_output_file=out, batch_size=512, engine_options=dict(eo, tokenize=mode),
                                sweep="arrays")
            finally:
                pm.load_archive = load
            jobs[mode].append(n / (time.perf_counter() - t0 - archive_s[0]))
            import hashlib
            files.setdefault(mode, hashlib.sha256(open(out, "rb").read()).hexdigest())
    print("test_siamese(sweep=\"arrays\"), issue reports/s whole job without the archive load (read + tokenise + anchors + score + records + metrics), alternating:")
    for mode in ("host", "gpu"):
        print("  tokenize=%-4s %s" % (mode, "  ".join("%8.0f" % r for r in jobs[mode])))
    s2 = spread(jobs["host"], jobs["gpu"])
    ok2 = np.mean(jobs["gpu"]) >= np.mean(jobs["host"]) - s2
    print("  gpu / host = %.3f (means); repeat-to-repeat spread %.0f reports/s; predictions files identical: %s" % (np.mean(jobs["gpu"]) / np.mean(jobs["host"]), s2, files["host"] == files["gpu"]))
    print("  STATEMENT 2 — the whole-job rate with gpu is not lower than with host by more than that spread: %s" % ("PASS" if ok2 else "FAIL"), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child-host":
        child_host(sys.argv[2])
    else:
        main()
