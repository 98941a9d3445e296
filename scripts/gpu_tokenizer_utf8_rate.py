"""What the UTF-8 mode of the device WordPiece tokenizer (MEMVUL_TOKENIZE=gpu-utf8) buys, measured: ``batch_ids`` with a share s of the reports carrying one
non-ASCII fragment each.  The 40 k-report corpus and the synthetic 30 522-entry vocabulary of scripts/gpu_tokenizer_rate.py; s in {0, 0.1, 0.3, 1}; the
fragments are those of the tests' edge list (tests/wordpiece_utf8_kit.py FRAGMENTS), appended to report i when frac(i x golden ratio) < s; three alternating
repeats of everything.

  batch_ids texts/s, 16 384-text chunks: host (the threads the box gives), host with RAYON_NUM_THREADS=2 (a child process of its own: the Rust thread pool is
      sized once), gpu (ASCII rows on the device, the rest on the host), gpu-utf8 (every row to the device)
  at s = 0: the kernel's own time per chunk (HIP events, mv_tok_kernel_ms) for wp_encode_kernel and wp_encode_u8_kernel on the same packed chunks

WHAT IT IS HELD TO (printed as PASS / FAIL against the repeat-to-repeat spread of the two rates compared, never against a fixed figure):
  1. at every s > 0, gpu-utf8 is not slower than gpu;
  2. at s = 0, gpu-utf8 is within the spread of gpu.
Usage (GPU box): python scripts/gpu_tokenizer_utf8_rate.py [N] > profiles/gpu_tokenizer_utf8_bench.txt"""
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

from gpu_tokenizer_rate import CHUNK, rate, spread, texts_of, tokenizer  # noqa: E402

SHARES = (0.0, 0.1, 0.3, 1.0)


def with_share(texts, s):
    from wordpiece_utf8_kit import FRAGMENTS

    frags = [f for f in FRAGMENTS if len(f) < 40]
    return [t + " " + frags[i % len(frags)] if (i * 0.6180339887498949) % 1.0 < s else t for i, t in enumerate(texts)]


def child_host(test_path):
    texts, tok = texts_of(test_path), tokenizer()
    rate(tok, texts[:2048])
    print(json.dumps({str(s): [rate(tok, with_share(texts, s)) for _ in range(3)] for s in SHARES}))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40000
    import plumbing_util as pu
    import r06_e2e_dropin as e2e

    rng = np.random.default_rng(11)
    root = pu.make_fixture(n_irs=4, n_anchors=4, layers=2)[0]
    vocab = os.path.join(root, "vocab.txt")
    words = e2e.make_vocab(vocab, rng)
    os.environ["MEMVUL_BERT_VOCAB"] = vocab
    os.environ.pop("MEMVUL_ALLOW_HASH_TOKENIZER", None)
    os.environ.pop("MEMVUL_TOKENIZE", None)
    _, test_path = e2e.make_corpus(root, rng, words, n)
    texts = texts_of(test_path)
    print("N = %d issue reports (%.1f MB of text), chunks of %d, max_length 256, host cores %d, tokenizers' thread pool: the box's default"
          % (n, sum(map(len, texts)) / 1e6, CHUNK, os.cpu_count()), flush=True)

    t0 = time.perf_counter()
    host, gpu, u8 = tokenizer(), tokenizer().attach_device(0), tokenizer().attach_device(0, unicode=True)
    print("attach (table build, %d of 131 072 code points covered, and upload included): %.2f s" % (int(u8._code_points["covered"].sum()), time.perf_counter() - t0), flush=True)
    env = dict(os.environ, RAYON_NUM_THREADS="2")
    host2 = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--child-host", test_path], env=env, capture_output=True, text=True,
                                      check=True).stdout.strip().splitlines()[-1])
    ok1, ok2 = True, True
    for s in SHARES:
        rows = with_share(texts, s)
        a, b, c = host.batch_ids(rows[:4096]), gpu.batch_ids(rows[:4096]), u8.batch_ids(rows[:4096])
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
        for t in (gpu, u8):
            t.device_counts = {"device": 0, "literal": 0, "non_ascii": 0}
        r = {"host": [], "gpu": [], "gpu-utf8": []}
        for _ in range(3):
            r["host"].append(rate(host, rows))
            r["gpu"].append(rate(gpu, rows))
            r["gpu-utf8"].append(rate(u8, rows))
        sp = spread(r["gpu"], r["gpu-utf8"])
        print("s = %.1f (%d of %d reports with a non-ASCII fragment), batch_ids texts/s, three alternating repeats:" % (s, sum(not t.isascii() for t in rows), n))
        print("  host, default threads     %s" % "  ".join("%8.0f" % x for x in r["host"]))
        print("  host, RAYON_NUM_THREADS=2 %s" % "  ".join("%8.0f" % x for x in host2[str(s)]))
        print("  gpu                       %s   rows: %s" % ("  ".join("%8.0f" % x for x in r["gpu"]), gpu.device_counts))
        print("  gpu-utf8                  %s   rows: %s" % ("  ".join("%8.0f" % x for x in r["gpu-utf8"]), u8.device_counts))
        print("  gpu-utf8 / gpu = %.3f, gpu-utf8 / host = %.2f, gpu-utf8 / host at two threads = %.2f (means); spread of gpu and gpu-utf8 %.0f texts/s"
              % (np.mean(r["gpu-utf8"]) / np.mean(r["gpu"]), np.mean(r["gpu-utf8"]) / np.mean(r["host"]), np.mean(r["gpu-utf8"]) / np.mean(host2[str(s)]), sp), flush=True)
        if s > 0:
            ok = np.mean(r["gpu-utf8"]) >= np.mean(r["gpu"]) - sp
            ok1 &= bool(ok)
            print("    gpu-utf8 not slower than gpu by more than the spread: %s" % ("yes" if ok else "NO"))
        else:
            ok2 = bool(abs(np.mean(r["gpu-utf8"]) - np.mean(r["gpu"])) <= sp)
    print("STATEMENT 1 — at every s > 0, gpu-utf8 is not slower than gpu: %s" % ("PASS" if ok1 else "FAIL"))
    print("STATEMENT 2 — at s = 0, gpu-utf8 is within the spread of gpu: %s" % ("PASS" if ok2 else "FAIL"), flush=True)

    packed = []
    for i in range(0, len(texts), CHUNK):
        rows = texts[i:i + CHUNK]
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(t) for t in rows], out=off[1:])
        packed.append(("".join(rows).encode("ascii"), off))
    ms = {"wp_encode_kernel": [], "wp_encode_u8_kernel": []}
    for _ in range(3):
        for p, o in packed:
            if len(o) - 1 != CHUNK:
                continue
            x = u8._device.encode(p, o, 256, True)
            ms["wp_encode_kernel"].append(u8._device.kernel_ms())
            y = u8._device.encode_u8(p, o, 256, True)
            ms["wp_encode_u8_kernel"].append(u8._device.kernel_ms())
            assert all(a.tobytes() == b.tobytes() for a, b in zip(x, y))
    for k, v in ms.items():
        print("s = 0, %-20s own time per %d-text chunk (HIP events): min %.2f ms, median %.2f ms, max %.2f ms = %.0f texts/s at the median"
              % (k, CHUNK, min(v), np.median(v), max(v), CHUNK / (np.median(v) / 1e3)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child-host":
        child_host(sys.argv[2])
    else:
        main()
