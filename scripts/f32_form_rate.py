"""The rate of the fp32 reference form (compute dtype "f32", include/memvul_hip.h MV_F32) at the bench shape — B 256 issue reports x S 256 tokens against G 124
anchors — with its per-class HIP-event times, and the FFN-1 launch alone in TF against the 155 TF the fp32-input MFMA sustains and the 122 TF an untuned
LDS-tiled GEMM reaches on it.  There is no gate: the form exists so that an audit finishes in seconds where the CPU reference takes hours.
Usage: python scripts/f32_form_rate.py [--steps 3] [--out profiles/f32_form_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memvul_amd import synth  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402

B, S, G = 256, 256, 124
FLOP_PER_TOKEN = 12 * 2 * (768 * 2304 + 768 * 768 + 2 * 768 * 3072)  # the four GEMMs of 12 layers (attention: + 2 x 2 x S x 768 per token and layer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dims = synth.BertDims(layers=12)
    w = synth.make_weights(dims)
    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=B * S, max_batch=B, max_anchors=128)
    eng.load_state_dict(w, "f32")
    ids, lens = synth.make_ids(B, S, dims.vocab_size)
    aids, alens = synth.make_ids(G, 64, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=8)
    eng.anchor_append(aids, alens)
    eng.forward(ids, lens, want_logits=False, want_probs=False)  # warm-up
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.forward(ids, lens, want_logits=False, want_probs=False)
    dt = (time.perf_counter() - t0) / args.steps
    say(f"fp32 form, B {B} x S {S} x G {G} (the planes fit: B not reduced): {dt * 1e3:.1f} ms per batch, {B / dt:.0f} issue reports/s, "
        f"{B * S * FLOP_PER_TOKEN / dt / 1e12:.1f} TF over the GEMM FLOPs")
    eng.profile_enable(True)
    eng.forward(ids, lens, want_logits=False, want_probs=False)
    prof = eng.profile_read()
    eng.profile_enable(False)
    total = sum(ms for ms, n in prof.values())
    for name, (ms, n) in prof.items():
        if n:
            say(f"  {name:16s} {ms:9.3f} ms  {n:4d} launches  {100 * ms / total:5.1f} %")
    ms1, n1 = prof["gemm_ffn1_gelu"]
    say(f"FFN-1 in the pass: {2 * B * S * 768 * 3072 * n1 / ms1 / 1e9:.1f} TF per launch")
    rng = np.random.default_rng(0)
    A = rng.standard_normal((B * S, 768)).astype(np.float32)
    W = (rng.standard_normal((3072, 768)) * 0.05).astype(np.float32)
    _, ms = eng.test_gemm_f32(A, W, np.zeros(3072, np.float32), act="gelu", iters=10)
    say(f"FFN-1 alone (M {B * S}, N 3072, K 768, 10 launches back to back): {ms:.3f} ms, {2 * B * S * 768 * 3072 / ms / 1e9:.1f} TF "
        "(instruction: 155 TF sustained; untuned LDS-tiled GEMM on it: 122 TF)")
    A2 = rng.standard_normal((B * S, 3072)).astype(np.float32)
    W2 = (rng.standard_normal((768, 3072)) * 0.05).astype(np.float32)
    _, ms = eng.test_gemm_f32(A2, W2, np.zeros(768, np.float32), A[:, :768].copy(), act="res", iters=10)
    say(f"FFN-2 alone (M {B * S}, N 768, K 3072): {ms:.3f} ms, {2 * B * S * 768 * 3072 / ms / 1e9:.1f} TF")
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
