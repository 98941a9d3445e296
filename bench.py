#!/usr/bin/env python
"""bench.py — issue-reports/sec of the MemVul predict_memory.py hot loop on MI355X.

One "step" = one pass of the hot path (BERT issue-encoder forward + CWE anchor-memory match,
model_memory.py:133-147) over one batch of synthetic issue reports.  Workload = BASELINE.json
configs[1]: bert-base-uncased geometry, seq_len 256, batch 256, 124-anchor memory.  Inputs are resident in HBM when
the timed region starts (mv_corpus_upload); weights are seeded random init.

The headline `value` is measured in the FASTEST compute dtype whose logit error on trained-like weights, MEASURED IN THIS RUN
against the CPU leg, is within the reference's 1e-3 tolerance (`--compute auto`, the default): MV_F16X8 (fp16 MFMA sweep + one
fp8 correction sweep per GEMM, fp32 accumulate) unless MV_F16 passes too.  The other mode rides along as the `fast` (MV_F16) or
`precise` object with its own error stated.

    python bench.py                              # 1 GPU
    python bench.py --full                       # + every other leg (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 with `metric`, `value`, `unit`, `higher_is_better`, `dtype` and `ms_per_step` (wall time of one
of the K timed steps).  A plain run does only that: set-up, W warm-up steps, the K timed steps, the line; without the CPU leg
`--compute auto` is MV_F16X8 (MV_F16 misses the 1e-3 contract on trained-like weights by ~5x, so auto never hands it `value`).
`--dump-outputs DIR` writes the last timed step's results as .npy files (seeded inputs: identical from run to run).
`--full` adds `roofline` (dominant kernel: algorithmic FLOPs per launch / HIP-event duration on the engine's stream),
`cpu_baseline` (the reference's CPU graph, oracle/hf_reference.py, timed on the host cores on a bounded sample, with and
without the reference's per-batch host work), `contract` (both modes' trained-like logit errors and which mode carries `value`),
and — N = 1 — `fast` (the other compute dtype on the same workload) and `cfg3` (BASELINE.json configs[2]: S 512, B 128);
N > 1 — `corpus_shard`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from memvul_amd import synth  # noqa: E402
from memvul_amd import distributed as mvdist  # noqa: E402

if os.environ.get("MEMVUL_BENCH_STUB_ENGINE"):
    # CPU regression test of this file's N > 1 control flow and JSON contract (tests/test_distributed_cpu.py): a numpy stand-in
    # with the Engine surface, NO GPU, NO measurement — the line says so in `data` and `config.note`
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from bench_stub_engine import Engine  # noqa: E402
else:
    from memvul_amd.binding import Engine  # noqa: E402

MFMA_PEAK_TFLOPS = 2500.0  # MI355X dense fp16/bf16 MFMA peak (MI355X_MICROARCH.md)
LOGIT_TOL = 1e-3           # BASELINE.json north_star: logits within 1e-3 of the reference CPU path
DEFAULT_CLS_ASIDE = "1"    # the library's default of MEMVUL_CLS_ASIDE (engine.hip mv_handle::cls_aside)
AUTO_MARGIN = 0.5          # --compute auto hands `value` to MV_F16 only if its measured trained-like error is <= AUTO_MARGIN * LOGIT_TOL
MODE_DTYPE = {"f16": "fp16 (MV_F16: fp16 MFMA operands, fp32 accumulate)",
              "precise": "fp16 + fp8 (MV_F16X8: fp16 MFMA sweep + one OCP-e4m3 MFMA correction sweep per GEMM, fp32 accumulate)"}
H, I, P = 768, 3072, 512
GEMM_CLASSES = ("gemm_qkv", "gemm_attn_out", "gemm_ffn1_gelu", "gemm_ffn2")
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_current.json")
LIB_STAMP = os.path.join(ROOT, "memvul_amd", "lib", "libmemvul_hip.so.stamp")


def load_pmc(mode="precise"):
    """Counter-derived figures of the GEMM classes (HBM bytes per launch = 2 x FETCH_SIZE + WRITE_SIZE per the gfx950 correction;
    matrix-pipe busy fraction; effective shader clock) from the separate rocprofv3 --pmc passes of this workload
    (scripts/gpu_pmc.sh writes profiles/pmc_current.json together with the stamp of the library it profiled).  They are
    reported ONLY when the DEVICE CODE profiled is the device code loaded now (the stamp's `dev` line: sha256 of the gfx950
    code object in the .so; stamps without it are compared whole) — a kernel edit can never leave stale counter numbers in a
    bench line, a host-only edit of the library does not throw them away; otherwise `traffic` is null and
    the note says why."""
    def lines(stamp):
        return dict(line.split(" ", 1) for line in str(stamp).strip().splitlines() if " " in line)

    try:
        pmc = json.load(open(PMC_FILE))
        stamp = open(LIB_STAMP).read().strip()
    except Exception as e:  # no counter pass on record / no stamp next to the library
        return {}, "no counter pass on record (%s)" % type(e).__name__
    have, want = lines(pmc.get("lib_stamp")), lines(stamp)
    same = have.get("dev") == want["dev"] if ("dev" in have and "dev" in want) else pmc.get("lib_stamp") == stamp
    if not same:
        return {}, "profiles/pmc_current.json was taken on other device code than the loaded libmemvul_hip.so (%s..., loaded %s...): not reported" % (
            str(have.get("dev") or have.get("src"))[:12], str(want.get("dev") or want.get("src"))[:12])
    classes = pmc.get("classes_by_mode", {}).get(mode)
    if classes is None:
        return {}, "profiles/pmc_current.json holds no counter pass of the %s mode" % mode
    return classes, "profiles/pmc_current.json (rocprofv3 --pmc, same workload and compute dtype, separate passes, device code %s...)" % str(
        want.get("dev") or want.get("src"))[:12]


def flops_per_ir(S: int, G: int, layers: int = 12) -> float:
    """Algorithmic FLOPs of one issue report."""
    per_layer = 24 * S * H * H + 4 * S * S * H
    return layers * per_layer + 2 * H * H + 2 * H * P + G * 7680.0


def executed_flops_per_ir(S: int, G: int, layers: int = 12, cls_prune: bool = True) -> float:
    """FLOPs the engine executes per issue report.  With last-layer pruning (only hidden[:, 0] reaches the pooler,
    model_memory.py:99) the last layer is the K and V projections of every token plus one query row per head and
    the [CLS] row through the output projection and the FFN."""
    if not cls_prune or layers == 0:
        return flops_per_ir(S, G, layers)
    per_layer = 24 * S * H * H + 4 * S * S * H
    last = 4 * S * H * H + 4 * S * H + 20 * H * H
    return (layers - 1) * per_layer + last + 2 * H * H + 2 * H * P + G * 7680.0


def gemm_flops(cls: str, M: int) -> float:
    return {"gemm_qkv": 2.0 * M * H * 3 * H, "gemm_attn_out": 2.0 * M * H * H, "gemm_ffn1_gelu": 2.0 * M * H * I,
            "gemm_ffn2": 2.0 * M * I * H}[cls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--anchors", type=int, default=124)
    ap.add_argument("--anchor-len", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--full", action="store_true", help="also run everything besides the headline: the trained-like error contract (CPU leg), the "
                    "per-kernel HIP-event passes, the sustained rate, the matcher, the CPU baseline, cfg3 and the second compute dtype (N = 1), "
                    "the corpus-shard leg (N > 1); --cpu-sample, --ab, --no-profile, --ragged, --no-precise, --sustain-s, --shard-irs and "
                    "--matcher-anchors shape those legs and act only with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step computed (its batch's "
                    "`best` [B, 2] and `best_idx` [B]) as DIR/<name>.npy, float32 / float64")
    ap.add_argument("--cpu-sample", type=int, default=192, help="IRs timed on the CPU baseline (three batches of 64; bounded at ~30 s; 0 disables)")
    ap.add_argument("--ab", action="store_true", help="N = 1: also run the both-terms form of the precise mode (MEMVUL_CLS_ASIDE=0) on the same workload: the "
                    "`precise_cls_aside_off` object (ledger material, not part of the default line)")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event passes (no `roofline` / `kernels`)")
    ap.add_argument("--ragged", action="store_true", help="also time a ragged corpus (lengths uniform in [16, seq_len]) swept "
                    "padded to seq_len and length-bucketed (each batch at its longest member); adds a `ragged` object")
    ap.add_argument("--streams", type=int, default=2, choices=(1, 2), help="batches of the resident sweep in flight at once")
    ap.add_argument("--compute", default="auto", choices=("auto", "f16", "fast", "f16x8", "precise"), help="compute dtype of the headline `value`; auto = "
                    "the fastest mode whose trained-like logit error measured in this run is <= 1e-3 (precise when the CPU leg is off, as it is "
                    "without --full); precise = f16x8 = MV_F16X8 (+ one fp8 correction sweep per GEMM: holds 1e-3 on trained-like logits); "
                    "f16 = fast = MV_F16; the --full line carries the other mode as its `fast` / `precise` object either way")
    ap.add_argument("--no-precise", "--no-second", dest="no_second", action="store_true", help="N = 1: skip the second engine (the `fast` / "
                    "`precise` object of the mode that does not carry `value`) and the `cfg3` object")
    ap.add_argument("--sustain-s", type=float, default=3.0, help="N = 1: also report the rate over a run of at least this many seconds (0 disables)")
    ap.add_argument("--shard-irs", type=int, default=0, help="N > 1: issue reports per rank in the corpus-shard leg (0 = ceil(1221677 / 8), the "
                    "8-GPU shard of the reference's corpus, README.md:8; -1 disables)")
    ap.add_argument("--matcher-anchors", type=int, default=1000, help="N = 1: anchors of the fused match + top-k measurement (configs[4]; 0 disables)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:  # a plain run: set up, warm up, the timed steps, the headline line — nothing else
        args.cpu_sample, args.no_profile, args.sustain_s, args.matcher_anchors = 0, True, 0.0, 0
        args.no_second, args.ab, args.ragged, args.shard_irs = True, False, False, -1

    # `--gpus N` is a promise about the line's `n_gpus`: under a launcher WORLD_SIZE must say N too; WITHOUT a launcher this
    # process becomes the launcher of N ranks (self_launch) — it never runs one rank and reports it as N, or N as one
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args.gpus))
    rank, local_rank, world = mvdist.env_world()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: refusing to run (the line's n_gpus would not be what was asked for)")
    if args.cpu_sample > 0 and world == 1:
        import torch  # noqa: F401  (the CPU baseline leg only; loaded BEFORE the engine: see tests/test_gpu_parity.py)
    multi = world > 1
    # development check of the N > 1 control flow on a ONE-GPU box (not a measurement): every rank shares device 0 and the
    # exchange runs over the rendezvous hub instead of RCCL (one GPU cannot host two RCCL ranks); the JSON line says so
    one_gpu_smoke = multi and os.environ.get("MEMVUL_BENCH_ONE_GPU_SMOKE", "") != ""
    stub = bool(os.environ.get("MEMVUL_BENCH_STUB_ENGINE"))
    if one_gpu_smoke:
        local_rank = 0

    B, S, G, K, W = args.batch, args.seq_len, args.anchors, args.steps, args.warmup
    dims = synth.BertDims(layers=args.layers)
    weights = synth.make_weights(dims)
    # which compute dtype carries `value`: the fastest one whose trained-like logit error, measured HERE against the CPU leg, holds
    # the reference's tolerance (model_memory.py:133-147 at config_memory.json:38's temperature)
    contract = None
    if args.compute in ("f16", "fast"):
        mode = "f16"
    elif args.compute in ("f16x8", "precise"):
        mode = "precise"
    else:
        mode = "precise"
    if world == 1 and args.cpu_sample > 0 and not stub:
        contract = trained_like_errors(dims, S)
        if args.compute == "auto":
            # the sample is small (16 IRs x 8 anchors: a max over 128 logit pairs moves +-40 % with the draw), so the fast mode only
            # takes the headline with a 2x margin to the tolerance — `value` cannot flip meaning between runs on a borderline reading
            mode = "f16" if contract["logit_max_abs_err_trained_like"]["f16"] <= AUTO_MARGIN * LOGIT_TOL else "precise"
    eng = Engine(local_rank, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=max(B * S, 128 * 512),
                 max_batch=max(B, 256), max_anchors=max(G, 1024))
    eng.load_state_dict(weights, mode)
    eng.set_streams(args.streams)
    transport, comm_info = "none (one rank)", {}
    if multi:
        # the N > 1 transport: the ranks agree over a rendezvous hub whether RCCL bound inside libmemvul_hip.so (mv_comm_*,
        # collective on the engine's stream, no torch in the process) carries the statistics or the hub itself does
        # (MEMVUL_BENCH_ONE_GPU_SMOKE=rccl lets the shared-GPU ranks TRY RCCL: ncclCommInitRank refuses two ranks on one device,
        # so the run exercises the agreement's fall-back — every rank reports the failure, all move to the hub together)
        skip_rccl = stub or (one_gpu_smoke and os.environ.get("MEMVUL_BENCH_ONE_GPU_SMOKE") != "rccl")
        try:
            transport = mvdist.init_transport(eng, rank, world, prefer="tcp" if skip_rccl else "rccl")
        except mvdist.HubPortInUse as e:  # (rank 0 only; the other ranks are ended by the launcher, which retries on another port pair)
            print("bench.py: " + str(e), file=sys.stderr)
            raise SystemExit(mvdist.EXIT_PORT_IN_USE)
        # what RCCL itself says about the communicator the statistics travel over (mv_comm_info: ncclCommCount / ncclGetVersion)
        comm_info = eng.comm_info() if hasattr(eng, "comm_info") else {}
        if transport.startswith("rccl") and comm_info.get("rccl_ranks") != world:
            raise SystemExit(f"transport says RCCL but ncclCommCount reports {comm_info.get('rccl_ranks')} ranks for WORLD_SIZE={world}")
        if mvdist.transport_world() != world:
            raise SystemExit(f"the agreed transport spans {mvdist.transport_world()} ranks for WORLD_SIZE={world}")

    # anchor memory: G synthetic CWE descriptions of up to 512 tokens, built once per process (untimed;
    # predict_memory.py:81-83 forwards them in chunks of 128)
    aids, alens = synth.make_ids(G, args.anchor_len, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=32)
    for s0 in range(0, G, 128):
        LA = int(alens[s0:s0 + 128].max())
        eng.anchor_append(aids[s0:s0 + 128, :LA], alens[s0:s0 + 128])

    # this rank's shard of the synthetic corpus, resident in HBM before the clock starts
    n_batches = min(K + W, 16)
    ids, lens = synth.make_ids(n_batches * B, S, dims.vocab_size, seed=synth.SEED + 1000 * rank)
    eng.corpus_upload(ids, lens)

    def step(i):
        eng.corpus_run((i % n_batches) * B, B, B, keep_probs=False)

    for i in range(W):
        step(i)
    eng.sync()
    if multi:
        mvdist.all_gather_stats(np.zeros(4, np.float32), np.zeros(4, np.uint8))  # RCCL communicator warm-up
        mvdist.barrier()
    # per-kernel breakdown: a separate, untimed pass with ONE batch in flight and HIP events around every launch
    # (with two batches in flight a launch's event span includes the time it shares the chip with the other batch's
    # kernels, so it says nothing about the kernel)
    breakdown, dom = {}, None
    if not args.no_profile:
        eng.set_streams(1)
        eng.profile_enable(True)
        eng.profile_select(None)
        eng.profile_read()
        for i in range(min(K, 4)):
            step(i)
        breakdown = eng.profile_read()
        gem = {k: v for k, v in breakdown.items() if k.startswith("gemm_") and k in GEMM_CLASSES and v[1]}
        dom = max(gem, key=lambda k: gem[k][0])
        eng.profile_enable(False)
    eng.set_streams(args.streams)
    lab = synth.make_labels(n_batches * B, seed=synth.SEED + rank)
    if multi:
        mvdist.barrier()
    eng.sync()
    t0 = time.perf_counter()
    for i in range(K):
        step(W + i)
    # whole job: per-IR results of the resident sweep back to the host, then the single exchange step
    best, idx, _ = eng.corpus_results(0, n_batches * B)  # synchronises the stream
    t_gather0 = time.perf_counter()
    all_s, all_l = mvdist.all_gather_stats(best[:, 0], lab) if multi else (best[:, 0], lab)
    gather_ms = (time.perf_counter() - t_gather0) * 1e3
    if multi:
        mvdist.barrier()
    t1 = time.perf_counter()
    elapsed = mvdist.all_reduce_max(t1 - t0) if multi else (t1 - t0)
    if args.dump_outputs and rank == 0:
        last = ((W + K - 1) % n_batches) * B  # the corpus rows the last timed step scored
        dump_outputs(args.dump_outputs, best=best[last:last + B], best_idx=idx[last:last + B])
    # roofline pass: the same K steps once more with one batch in flight and HIP events (engine stream) around the
    # dominant GEMM class only -> per-launch duration of that kernel alone, and the one-batch-in-flight rate
    prof, single_rate = {}, None
    if not args.no_profile:
        eng.set_streams(1)
        eng.profile_enable(True)
        eng.profile_select([dom])
        eng.profile_read()
        eng.sync()
        ts0 = time.perf_counter()
        for i in range(K):
            step(W + i)
        eng.sync()
        single_rate = K * B / (time.perf_counter() - ts0)
        prof = eng.profile_read()
        eng.profile_enable(False)
        eng.profile_select(None)
        eng.set_streams(2 if args.streams == 2 else 1)

    # N > 1: the job BASELINE.json configs[3] names — a contiguous shard of the 1.22 M-IR corpus per rank, swept once, ONE
    # all-gather of the per-IR (score, label) statistics (every rank takes part; rank 0 reports)
    shard = corpus_shard_leg(eng, dims, B, S, rank, world, args.shard_irs) if multi else None
    # N = 1: a sustained (>= 3 s) rate next to the K-step figure (the chip is power-limited: short bursts run hotter)
    sustained = sustained_leg(eng, step, B, args.sustain_s) if (not multi and args.sustain_s > 0) else None

    if rank != 0:
        mvdist.shutdown()
        return
    from memvul_amd.custom_metric import threshold_confusion_table

    table = threshold_confusion_table(all_l, all_s)
    total_irs = world * K * B
    value = total_irs / elapsed
    M = B * S
    fpi = flops_per_ir(S, G, dims.layers)
    pruned = os.environ.get("MEMVUL_CLS_PRUNE", "1") != "0"
    fpi_exec = executed_flops_per_ir(S, G, dims.layers, pruned)
    out = {
        "metric": "issue-reports/sec at seq_len=%d (BERT-base issue encoder + %d-anchor memory match)" % (S, G),
        "value": round(value, 2), "unit": "issue-reports/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": round(elapsed / K * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": MODE_DTYPE[mode], "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[1]: 1xMI355X-per-rank, bert-base-uncased geometry (%d layers), "
                               "seq_len=%d, batch=%d, %d-anchor CWE memory, compute dtype %s; "
                               "seeded random-init weights, synthetic token ids resident in HBM" % (dims.layers, S, B, G,
                                                                                                 "MV_F16" if mode == "f16" else "MV_F16X8"),
                   "compute": mode,
                   "global_batch": world * B, "seq_len": S, "anchors": G, "parallelism": "dp%d (corpus shards, one "
                   "all-gather of (score,label) stats)" % world, "stats_transport": transport,
                   **({"comm_world": mvdist.transport_world(), "rccl_ranks": comm_info.get("rccl_ranks", 0),
                       "rccl_version": comm_info.get("rccl_version", 0),
                       "launcher": "bench.py self_launch (no WORLD_SIZE in the environment)" if os.environ.get("MEMVUL_SELF_LAUNCHED") else "external (WORLD_SIZE set)"}
                      if multi else {})},
        # executed FLOPs (with last-layer [CLS] pruning the fraction is priced on what runs)
        "e2e_tflops_per_gpu": round(value / world * fpi_exec / 1e12, 2),
        "e2e_mfma_frac": round(value / world * fpi_exec / 1e12 / MFMA_PEAK_TFLOPS, 4),
        "gflop_per_ir": {"algorithmic": round(fpi / 1e9, 3), "executed": round(fpi_exec / 1e9, 3), "last_layer_cls_pruning": pruned},
        "batches_in_flight": args.streams,
        # MV_F16X8: activation elements beyond the +-112 range of the fp8 correction planes over everything this engine ran (mv_x8_saturation)
        "x8_saturated_elements": (eng.x8_saturation() if (mode == "precise" and hasattr(eng, "x8_saturation")) else None),
        # MV_F16X8: the concentration monitor (mv_attention_concentration): largest collision mass of a [CLS] row on ORDINARY keys / items above 0.25 over everything this engine ran
        "attention_concentration": (dict(zip(("max_collision_on_ordinary_keys", "items_over_0.25", "items_total"), eng.attention_concentration()))
                                    if (mode == "precise" and hasattr(eng, "attention_concentration")) else None),
        "stats_allgather_ms": round(gather_ms, 3),
        "stats_table_sum": int(table.sum()),
    }
    if one_gpu_smoke:
        out["config"]["note"] = "MEMVUL_BENCH_ONE_GPU_SMOKE: all ranks share ONE GPU, exchange over the rendezvous hub: control-flow check, not a measurement"
    if stub:  # never a number that could be mistaken for a measurement: `value` is null, the stand-in's rate sits under its own name
        out["data"] = "stub"
        out["config"]["note"] = "MEMVUL_BENCH_STUB_ENGINE: numpy stand-in engine, NO GPU — a test of this file's control flow and JSON contract, not a measurement"
        out["stub_rate_not_a_measurement"] = out["value"]
        out["value"] = None
        for k in ("e2e_tflops_per_gpu", "e2e_mfma_frac"):
            out[k] = None
        prof = {}
    if prof:
        kernels = {}
        for name, (ms, n) in breakdown.items():
            if n:
                kernels[name] = {"ms_total": round(ms, 3), "launches": n, "avg_us": round(ms / n * 1e3, 2)}
                if name in GEMM_CLASSES:
                    kernels[name]["tflops"] = round(gemm_flops(name, M) / (ms / n * 1e-3) / 1e12, 1)
        ms, n = prof[dom]  # the dominant GEMM class, HIP events inside the timed region
        avg_us = ms / n * 1e3
        achieved = gemm_flops(dom, M) / (avg_us * 1e-6) / 1e12
        pmc, pmc_note = load_pmc(mode) if (B, S) == (256, 256) else ({}, "counter passes exist for the default workload only")
        cls = pmc.get(dom, {})
        out["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": round(achieved, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": cls.get("traffic_bytes"),
                           "flops_per_launch": gemm_flops(dom, M), "avg_launch_us": round(avg_us, 2), "launches_timed": n,
                           **{k: cls[k] for k in ("mfma_busy_frac", "effective_clock_ghz", "profiled_avg_us") if k in cls}, "pmc_source": pmc_note,
                           "note": "algorithmic FLOPs of the GEMM (in MV_F16X8 its fp8 correction sweep is overhead, not work) / HIP events around "
                                   "this kernel class over a pass of the same K steps with ONE batch in flight (`value` runs two: a launch's "
                                   "span then includes time shared with the other batch's kernels)"}
        out["value_one_batch_in_flight"] = round(world * single_rate, 2)
        out["kernels"] = kernels
        out["kernels_note"] = "per-class HIP-event breakdown from a separate untimed pass of %d steps, one batch in flight" % min(K, 4)
    if shard is not None:
        out["corpus_shard"] = shard
    if sustained is not None:
        out["value_sustained"] = sustained
    if args.ragged:
        out["ragged"] = ragged_leg(eng, dims, B, S, rank)
    if world == 1 and args.matcher_anchors > 0:
        out["matcher"] = matcher_leg(eng, args.matcher_anchors, B)
    if args.cpu_sample > 0 and world == 1 and not stub:
        out["cpu_baseline"], out["logit_max_abs_err_vs_cpu"], out["anchor_max_abs_err_vs_cpu"] = cpu_baseline(
            weights, dims, eng, ids, lens, S, args.cpu_sample, aids, alens)
    if contract is not None:
        errs = contract["logit_max_abs_err_trained_like"]
        out["logit_max_abs_err_trained_like"] = errs[mode]
        out["contract"] = {"logit_tol": LOGIT_TOL, "headline_mode": mode, "meets": bool(errs[mode] <= LOGIT_TOL),
                           "selection": ("--compute auto: MV_F16 if its measured error <= %g x tol, else MV_F16X8" % AUTO_MARGIN if args.compute == "auto"
                                         else "--compute " + args.compute),
                           "selection_sample_logits": contract.get("sample_logits"),
                           **contract}
    if world == 1 and not args.no_second and not stub:
        out["cfg3"] = cfg3_leg(eng, dims, mode, min(K, 10), W, args.streams, profile=not args.no_profile)
        eng.close()
        other = "f16" if mode == "precise" else "precise"
        out["fast" if other == "f16" else "precise"] = second_mode_leg(args, other, dims, weights, aids, alens, ids, lens, contract)
        if args.ab:  # the [CLS]-row A-side form (MEMVUL_CLS_ASIDE, engine.hip cls_aside): whichever of the two forms is NOT the library's default in this run
            other_cls = "0" if os.environ.get("MEMVUL_CLS_ASIDE", DEFAULT_CLS_ASIDE) == "1" else "1"
            out["precise_cls_aside_" + ("off" if other_cls == "0" else "on")] = precise_option_leg(args, dims, weights, aids, alens, ids, lens, S, {"MEMVUL_CLS_ASIDE": other_cls})
    print(json.dumps(out), flush=True)
    mvdist.shutdown()


def dump_outputs(out_dir, **arrays):
    """--dump-outputs: each array as out_dir/<name>.npy, floats as float32, integers as float64 (exact for int32)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32 if a.dtype.kind == "f" else np.float64))


def visible_gpus() -> int:
    """GPUs a rank could open (mv_device_count of the library; the stand-in engine has as many as it is asked for).  Counted in a short-lived
    child process: the launcher itself never loads the HIP runtime (it only spawns the ranks)."""
    if os.environ.get("MEMVUL_BENCH_STUB_ENGINE"):
        return 1 << 30
    import subprocess

    r = subprocess.run([sys.executable, "-c", "from memvul_amd.binding import device_count; print(device_count())"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    try:
        return int(r.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        print("bench.py: could not count the GPUs: " + r.stderr.strip()[-500:], file=sys.stderr)
        return 0


def free_port_pair(tries: int = 32) -> int:
    """A port P on 127.0.0.1 with P (MASTER_PORT) AND P + 1 (the rendezvous hub of memvul_amd/distributed.py) both bindable right now.  The probe
    sockets are closed before the ranks bind, so another process can still take one in between — the hub then fails with EADDRINUSE and the
    launch is retried with another pair (self_launch)."""
    import socket

    for _ in range(tries):
        with socket.socket() as s0:
            s0.bind(("127.0.0.1", 0))
            port = s0.getsockname()[1]
            if port >= 65535:
                continue
            with socket.socket() as s1:
                try:
                    s1.bind(("127.0.0.1", port + 1))
                except OSError:
                    continue
            return port
    raise RuntimeError("no free port pair on 127.0.0.1")


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` with no launcher in the environment: spawn the N ranks ourselves — one process per GPU, the
    same command line, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT / MEMVUL_RUN_TOKEN as `torch.distributed.run`
    would set them (rendezvous on 127.0.0.1) — and return the job's exit code: 0 only if EVERY rank exited 0 (rank 0 prints the
    one JSON line on this process's stdout; the other ranks' stdout goes to stderr).  Fewer than N visible GPUs: a message and a
    non-zero code, nothing is run (MEMVUL_BENCH_ONE_GPU_SMOKE, the shared-GPU control-flow check, is the one exception).
    One failed rank ends the others (by their PIDs) instead of leaving them in the rendezvous."""
    import secrets
    import subprocess

    have = visible_gpus()
    if have < n and not os.environ.get("MEMVUL_BENCH_ONE_GPU_SMOKE"):
        print(f"bench.py: --gpus {n} but only {have} GPU(s) visible to this process: not running "
              f"(a {have}-GPU line must be asked for with --gpus {max(have, 1)})", file=sys.stderr)
        return 2
    rc = 0
    for attempt in range(3):  # (a port of the pair taken between the probe and the ranks' bind: exit code EXIT_PORT_IN_USE of rank 0 -> another pair)
        port = free_port_pair()
        env0 = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MEMVUL_SELF_LAUNCHED="1")
        env0.setdefault("MEMVUL_RUN_TOKEN", secrets.token_hex(16))
        env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs = []
        for r in range(n):
            env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=None if r == 0 else sys.stderr))
        rc, live = 0, set(range(n))
        try:
            while live:
                for r in sorted(live):
                    c = procs[r].poll()
                    if c is None:
                        continue
                    live.discard(r)
                    if c != 0 and rc == 0:
                        rc = c if c > 0 else 1
                        print(f"bench.py: rank {r} of {n} exited with code {c}: ending the other ranks", file=sys.stderr)
                        for o in live:
                            procs[o].terminate()
                time.sleep(0.05)
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        if rc != mvdist.EXIT_PORT_IN_USE:
            break
        print(f"bench.py: port {port + 1} was taken before the rendezvous hub could bind it: retrying with another pair", file=sys.stderr)
    return rc


def precise_option_leg(args, dims, weights, aids, alens, ids, lens, S, switches):
    """MV_F16X8 under a set of library switches (read at mv_create): the same K steps on the same workload, and the trained-like logit error of
    that form against the CPU leg measured here (the same sample as `contract`)."""
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        B, G, K, W = args.batch, args.anchors, args.steps, args.warmup
        res = {"switch": " ".join("%s=%s" % kv for kv in sorted(switches.items()))}
        if args.cpu_sample > 0:
            res["logit_max_abs_err_trained_like"] = trained_like_errors(dims, S, modes=("precise",))["logit_max_abs_err_trained_like"]["precise"]
            res["meets_contract"] = bool(res["logit_max_abs_err_trained_like"] <= LOGIT_TOL)
        eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=max(B * S, 128 * 512), max_batch=max(B, 256), max_anchors=max(G, 1024))
        eng.load_state_dict(weights, "precise")
        eng.set_streams(args.streams)
        for s0 in range(0, G, 128):
            LA = int(alens[s0:s0 + 128].max())
            eng.anchor_append(aids[s0:s0 + 128, :LA], alens[s0:s0 + 128])
        eng.corpus_upload(ids, lens)
        nb = len(lens) // B

        def step(i):
            eng.corpus_run((i % nb) * B, B, B, keep_probs=False)

        for i in range(W):
            step(i)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(K):
            step(W + i)
        eng.corpus_results(0, nb * B)
        dt = time.perf_counter() - t0
        res.update(value=round(K * B / dt, 2), unit="issue-reports/s", ms_per_step=round(dt / K * 1e3, 4))
        if not args.no_profile:
            res["kernels_avg_us"], _ = mode_profile(eng, step, K, B * S, S, G, dims.layers)
            eng.set_streams(args.streams)
        res["x8_saturated_elements"] = eng.x8_saturation()
        eng.close()
        return res
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sustained_leg(eng, step, B, seconds):
    """The same steps for at least `seconds` of wall time: what the part sustains once it sits at its power limit."""
    eng.sync()
    t0 = time.perf_counter()
    n = 0
    while True:
        for i in range(16):
            step(n + i)
        n += 16
        eng.sync()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    return {"value": round(n * B / dt, 2), "unit": "issue-reports/s", "seconds": round(dt, 2), "steps": n}


def corpus_shard_leg(eng, dims, B, S, rank, world, shard_irs):
    """BASELINE.json configs[3]: each rank holds a contiguous shard of the corpus resident in HBM, sweeps it once (batches
    of B, two in flight), downloads its per-IR results once, then ONE RCCL all-gather of (score, label).  Communicator
    warm-up and the barriers sit outside the clock; the all-gather is inside it and timed on its own."""
    if shard_irs < 0:
        return None
    n = shard_irs if shard_irs > 0 else -(-1221677 // 8)
    rng_ids, lens = synth.make_ids(n, S, dims.vocab_size, seed=synth.SEED + 5000 + rank)
    lab = synth.make_labels(n, seed=synth.SEED + 9000 + rank)
    eng.corpus_upload(rng_ids, lens)
    del rng_ids
    eng.sync()
    mvdist.barrier()
    t0 = time.perf_counter()
    eng.corpus_run(0, n, B, keep_probs=False)
    eng.sync()
    t_compute = time.perf_counter() - t0
    best, idx, _ = eng.corpus_results(0, n)  # the one download of the shard's per-IR results (12 B per issue report)
    t_sweep = time.perf_counter() - t0
    tg = time.perf_counter()
    all_s, all_l = mvdist.all_gather_stats(best[:, 0], lab)
    gather_ms = (time.perf_counter() - tg) * 1e3
    t_rank = time.perf_counter() - t0
    elapsed = mvdist.all_reduce_max(t_rank)
    rates = mvdist.all_gather_rows(np.array([[n / t_sweep]], np.float32))[:, 0]  # every rank's own sweep rate, no collective in it
    total = int(len(all_s))
    return {"irs_per_rank": n, "irs_total": total, "value_corpus": round(total / elapsed, 2), "unit": "issue-reports/s",
            "seconds": round(elapsed, 3), "sweep_ms": round(t_compute * 1e3, 2), "results_d2h_ms": round((t_sweep - t_compute) * 1e3, 3),
            "allgather_ms": round(gather_ms, 3), "allgather_bytes_per_rank": int(n * 8),
            "fixed_overhead_frac": round(gather_ms * 1e-3 / elapsed, 5),
            "sum_of_rank_sweep_rates": round(float(rates.sum()), 2),
            "scaling_vs_sum_of_ranks": round(total / elapsed / float(rates.sum()), 4),
            "positives_gathered": int(all_l.sum()),
            # the gathered statistics in the order every rank holds them (rank-major: shard r's rows, then shard r + 1's) — a single process that
            # scored the eight shards one after the other hashes to the same value (tests/test_distributed_cpu.py, world 8)
            "stats_sha256": __import__("hashlib").sha256(np.ascontiguousarray(all_s, np.float32).tobytes() + np.ascontiguousarray(all_l, np.uint8).tobytes()).hexdigest(),
            "note": "per-rank shard = ceil(1,221,677 / 8) synthetic IRs x %d tokens unless --shard-irs says otherwise; value_corpus = all ranks' "
                    "IRs / max-over-ranks(sweep + result download + all-gather)" % S}


def matcher_leg(eng, G, B, k=10, reps=20):
    """BASELINE.json configs[4]: fused match + top-k over a G-anchor synthetic bank, measured as its own roofline
    (SURVEY.md §8d): algorithmic bytes 4 (B P + G P) + 8 B k against HBM, 2 B G P lane operations (the class-delta chain:
    sub + one fma; 5 B G P FLOP of the plain form) against the fp32 vector ALU's issue rate (match_topk.h).  HIP events on
    the engine's stream around the match (+ merge) launches."""
    bank = eng.anchor_get()
    rng = np.random.default_rng(3)
    u = np.maximum(rng.standard_normal((B, P)), 0).astype(np.float32) * np.float32(0.5)
    eng.anchor_set(synth.make_anchor_bank(G))
    eng.topk(u, k)
    eng.profile_enable(True)
    eng.profile_select(["match", "topk"])
    eng.profile_read()
    for _ in range(reps):
        eng.topk(u, k)
    prof = eng.profile_read()
    eng.profile_enable(False)
    eng.profile_select(None)
    eng.anchor_set(bank)
    us = (prof["match"][0] + prof["topk"][0]) / max(prof["match"][1], 1) * 1e3
    bytes_alg = 4 * (B * P + G * P) + 8 * B * k
    flop_plain = 5.0 * B * G * P            # sub, |.|*w (x2 classes) as the reference's concat + Linear would count them, + W_b.v
    laneops = 2.0 * B * G * P               # what the kernel issues per (b, g, feature): sub + one fma on the class-delta chain
    return {"anchors": G, "batch": B, "k": k, "avg_us": round(us, 2), "launches": {"match": prof["match"][1], "topk_merge": prof["topk"][1]},
            "bytes_algorithmic": bytes_alg, "GB_per_s": round(bytes_alg / (us * 1e-6) / 1e9, 1), "hbm_frac": round(bytes_alg / (us * 1e-6) / 8e12, 5),
            "valu_tflops": round(flop_plain / (us * 1e-6) / 1e12, 2), "valu_frac": round(flop_plain / (us * 1e-6) / 157.3e12, 4),
            "lane_ops_per_s_T": round(laneops / (us * 1e-6) / 1e12, 2),
            "note": "bound: fp32 VALU (arithmetic intensity %.0f FLOP/B >> the 20 FLOP/B vector ridge); P(same) [B, G] never reaches HBM, "
                    "only 8 B k bytes of results do" % (flop_plain / bytes_alg)}


def ragged_leg(eng, dims, B, S, rank, n_batches=16):
    """Real issue reports are not all seq_len tokens long.  The reference pads every batch to its longest member
    (predict_memory.py:97-101); the engine form is a corpus uploaded sorted by length and swept with mv_corpus_run_len.
    Times the same ragged synthetic corpus (lengths uniform in [16, S]) both ways, inputs resident before the clock starts."""
    n = n_batches * B
    ids, lens = synth.make_ids(n, S, dims.vocab_size, seed=synth.SEED + 77 + rank, ragged=True, min_len=16)
    res = {}
    eng.corpus_upload(ids, lens)
    for rep in range(2):  # first pass = warm-up
        eng.sync()
        t0 = time.perf_counter()
        eng.corpus_run(0, n, B)
        best_p, idx_p, _ = eng.corpus_results(0, n)
        res["padded_to_seq_len_irs"] = round(n / (time.perf_counter() - t0), 1)
    order = np.argsort(lens, kind="stable")
    sl = lens[order]
    eng.corpus_upload(ids[order], sl)
    for rep in range(2):
        eng.sync()
        t0 = time.perf_counter()
        for s0 in range(0, n, B):
            eng.corpus_run(s0, B, B, s_eff=int(sl[s0 + B - 1]))
        best_b, idx_b, _ = eng.corpus_results(0, n)
        res["length_bucketed_irs"] = round(n / (time.perf_counter() - t0), 1)
    inv = np.empty(n, np.int64)
    inv[order] = np.arange(n)
    res["max_abs_diff_best_prob"] = float(np.abs(best_b[inv] - best_p).max())
    res["mean_len"] = float(lens.mean())
    res["note"] = "same %d synthetic IRs, lengths uniform in [16, %d]; bucketed = sorted by length, each batch of %d run at its longest member's length rounded up to 64" % (n, S, B)
    return res


def reference_host_work(p, labels, urls, same_idx=0):
    """What the reference does on the HOST with every batch's probabilities, restated (model_memory.py:143, 169-191;
    allennlp evaluate's predictions file): the [B, G, 2] tensor becomes nested Python lists, every issue report gets a
    {anchor label: P(same)} dict by a Python loop over the anchors plus a deepcopy, and the batch's records are dumped as one
    JSON line.  Returns the serialized line (so the work cannot be optimised away)."""
    from copy import deepcopy

    probs = p.tolist()
    votes = {name: 0 for name in set(labels)}
    predict = []
    for row in probs:
        for pr, name in zip(row, labels):
            votes[name] = pr[same_idx]
        predict.append(deepcopy(votes))
    recs = [{"Issue_Url": urls[i], "label": "neg", "predict": predict[i]} for i in range(len(probs))]
    return json.dumps(recs)


def cpu_baseline(weights, dims, eng, ids, lens, S, n, aids, alens):
    """The reference's CPU graph (HF BertModel + pooler + header + matcher, fp32, host cores) on the first n IRs of the same
    synthetic corpus, timed twice over: the graph alone and with the reference's per-batch host work (reference_host_work) over
    all G anchors; also the GPU-vs-CPU logit error on those IRs against the first 16 anchors, which the CPU leg encodes itself
    (the other anchors' embeddings are taken from the engine: what is timed is the issue-report path; encoding all 124 anchors of up
    to 512 tokens on the host took 28 s of the default run)."""
    import torch

    from oracle.hf_reference import HFReference

    cores = os.cpu_count() or 1
    ref = HFReference(weights, dims.as_dict(), threads=min(cores, 32))
    bs = 8
    # the intra-op thread count that is fastest on this host (all cores is often slower on a many-core box): two batches of 8 per
    # candidate after one warm-up batch; then the anchors and the sample with it
    G = len(alens)
    v0 = np.zeros((G, P), np.float32)
    best_t, best_dt, calib = None, None, {}
    for t in sorted({c for c in (8, 16, 32, 64) if c <= cores} | {min(cores, 8)}):
        torch.set_num_threads(t)
        ref.predict(ids[:bs].astype(np.int64), np.ones((bs, S), bool), v0)
        t0 = time.perf_counter()
        for r in range(2):
            ref.predict(ids[r * bs:(r + 1) * bs].astype(np.int64), np.ones((bs, S), bool), v0)
        d = (time.perf_counter() - t0) / 2
        calib[t] = round(bs / d, 2)
        if best_dt is None or d < best_dt:
            best_t, best_dt = t, d
    torch.set_num_threads(best_t)
    bs_cal, bs = bs, 64  # the CPU leg runs at batch 64; the thread count was chosen on batches of 8 (bounded time)
    ta0 = time.perf_counter()
    GC = min(G, 16)   # anchors the CPU leg encodes itself (at the padded length of their chunk of 128, predict_memory.py:81-83)
    LA = int(alens[:128].max())
    vc = ref.instance_forward(aids[:GC, :LA].astype(np.int64), synth.mask_from_lens(alens[:GC], LA))
    anchor_s = time.perf_counter() - ta0
    v = eng.anchor_get()
    anchor_err = float(np.abs(v[:GC] - vc).max())
    v[:GC] = vc
    labels = ["CWE-%d" % (g % 97) for g in range(G)]
    t_graph, t_host, logits, done = 0.0, 0.0, [], 0
    for s0 in range(0, n, bs):
        part = ids[s0:s0 + bs].astype(np.int64)
        t0 = time.perf_counter()
        u, lg, p, best, idx = ref.predict(part, np.ones(part.shape, bool), v)
        t1 = time.perf_counter()
        line = reference_host_work(p, labels, ["https://example.invalid/issues/%d" % (s0 + i) for i in range(part.shape[0])])
        t2 = time.perf_counter()
        assert len(line) > part.shape[0] * G * 8
        t_graph += t1 - t0
        t_host += t2 - t1
        logits.append(lg)
        done += part.shape[0]
        if t_graph + t_host > 30.0:  # bounded sample
            break
    n = done
    logits = np.concatenate(logits)
    gpu = eng.forward(ids[:n], lens[:n])
    err = float(np.abs(gpu["logits"][:, :GC] - logits[:, :GC]).max())
    return ({"value": round(n / t_graph, 3), "with_host_loop": round(n / (t_graph + t_host), 3), "unit": "issue-reports/s", "cores": best_t,
             "host_cores": cores, "kind": "port", "thread_calibration_irs_per_s": calib, "thread_calibration_batch": bs_cal,
             "host_limits": host_limits(),
             "host_work_ms_per_ir": round(t_host / n * 1e3, 3), "anchor_bank_build_s": round(anchor_s, 2),
             "sample": f"{n} synthetic IRs x {S} tokens, batch {bs}, fp32 torch-CPU ({best_t} threads): HF BertModel (eager attention) + tanh "
                       f"pooler + ReLU header + bias-free matcher = the reference's CPU graph (AllenNLP itself is not installable here; "
                       f"the reference's own files run only in the build container, oracle/ref_harness); `with_host_loop` adds the "
                       f"reference's per-batch host work (p.tolist(), the B x G dict loop with deepcopy, json.dumps; model_memory.py:143, "
                       f"169-191) over all {G} anchors; the first {GC} anchors encoded by the CPU leg itself ({anchor_s:.0f} s, untimed): logits compared over those"},
            err, anchor_err)


def host_limits():
    """What bounds the CPU leg's parallelism on this box besides os.cpu_count(): the scheduler affinity of this process and the
    container's cgroup CPU quota (cpu.max: "<quota us> <period us>" or "max") — why a thread count far below the hardware thread
    count can be the fastest (threads beyond the quota only add contention)."""
    out = {}
    try:
        out["sched_affinity_cpus"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            out["cgroup_" + os.path.basename(path)] = open(path).read().strip()
        except Exception:
            pass
    try:
        out["loadavg_1m"] = os.getloadavg()[0]
    except Exception:
        pass
    return out


def trained_like_errors(dims, S, nt=16, gt=8, modes=("f16", "precise")):
    """max |logit error| of BOTH compute dtypes against the CPU leg (oracle/hf_reference.py, fp32) on the trained-like weights of
    SURVEY.md §8d (synth.make_weights(trained_like=True, match_scale=29): LayerNorm outlier dims, peaked attention, |logit| ~ 3):
    the measurement that decides which mode may carry `value` and that the line reports next to it."""
    import torch  # noqa: F401  (loaded before any engine exists)

    from oracle.hf_reference import HFReference

    wt = synth.make_weights(dims, qk_scale=2.0, match_scale=29.0, trained_like=True)
    ref = HFReference(wt, dims.as_dict(), threads=min(os.cpu_count() or 1, 16))
    ids, lens = synth.make_ids(nt, S, dims.vocab_size, seed=synth.SEED)
    ta, tl = synth.make_ids(gt, 512, dims.vocab_size, seed=synth.SEED + 1, ragged=True, min_len=32)
    LA = int(tl.max())
    v = ref.instance_forward(ta[:, :LA].astype(np.int64), synth.mask_from_lens(tl, LA))
    u, lg, p, best, idx = ref.predict(ids.astype(np.int64), np.ones((nt, S), bool), v)
    errs = {}
    for mode in modes:
        e2 = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=16 * 512, max_batch=16, max_anchors=16)
        e2.load_state_dict(wt, mode)
        e2.anchor_append(ta[:, :LA], tl)
        o = e2.forward(ids, lens)
        errs[mode] = float(np.abs(o["logits"] - lg).max())
        e2.close()
    return {"logit_max_abs_err_trained_like": errs, "sample_logits": int(lg.size),
            "trained_like_sample": ("%d IRs x %d tokens against %d anchors of up to %d tokens, %d-layer trained-like weights (LayerNorm outlier "
                                    "dims, peaked attention, matcher x29), max |logit| %.2f; CPU leg = oracle/hf_reference.py fp32" % (
                                        nt, S, gt, LA, dims.layers, float(np.abs(lg).max())))}


def mode_profile(eng, step, K, M, S, G, layers):
    """Per-class HIP-event breakdown (one batch in flight) of `step` on `eng` -> (kernels_avg_us, roofline of the dominant GEMM class)."""
    eng.set_streams(1)
    eng.profile_enable(True)
    eng.profile_select(None)
    eng.profile_read()
    for i in range(min(K, 4)):
        step(i)
    bd = eng.profile_read()
    eng.profile_enable(False)
    gem = {k: v for k, v in bd.items() if k in GEMM_CLASSES and v[1]}
    dom = max(gem, key=lambda k: gem[k][0])
    us = gem[dom][0] / gem[dom][1] * 1e3
    ach = gemm_flops(dom, M) / (us * 1e-6) / 1e12
    roof = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / MFMA_PEAK_TFLOPS, 4), "avg_launch_us": round(us, 2), "traffic": None,
            "note": "algorithmic FLOPs of the GEMM / its launch time (HIP events, one batch in flight; an fp8 correction sweep is not counted as work)"}
    return {k: round(v[0] / v[1] * 1e3, 2) for k, v in bd.items() if v[1]}, roof


def cfg3_leg(eng, dims, mode, K, W, streams, profile=True, B3=128, S3=512):
    """BASELINE.json configs[2] on the engine that carried `value` (same compute dtype): S = 512, B = 128 — rate, executed-FLOP
    fraction of the MFMA peak, the dominant GEMM class's roofline and the attention kernel's launch time (the S = 512 attention runs
    the chunked online-softmax form of attention_v2.h).  rocprofv3 evidence: profiles/r06_cfg3_precise_* (scripts/gpu_pmc.sh cfg3)."""
    nb = 8
    ids, lens = synth.make_ids(nb * B3, S3, dims.vocab_size, seed=synth.SEED + 303)
    eng.corpus_upload(ids, lens)
    eng.set_streams(streams)

    def step(i):
        eng.corpus_run((i % nb) * B3, B3, B3, keep_probs=False)

    for i in range(W):
        step(i)
    eng.sync()
    t0 = time.perf_counter()
    for i in range(K):
        step(W + i)
    eng.corpus_results(0, nb * B3)
    dt = time.perf_counter() - t0
    G = eng.n_anchors
    fpi_exec = executed_flops_per_ir(S3, G, dims.layers, cls_prune=os.environ.get("MEMVUL_CLS_PRUNE", "1") != "0")
    res = {"workload": "BASELINE.json configs[2]: seq_len=%d, batch=%d, %d anchors, compute dtype %s" % (S3, B3, G, "MV_F16" if mode == "f16" else "MV_F16X8"),
           "value": round(K * B3 / dt, 2), "unit": "issue-reports/s", "ms_per_step": round(dt / K * 1e3, 4), "steps": K,
           "e2e_mfma_frac": round(K * B3 / dt * fpi_exec / 1e12 / MFMA_PEAK_TFLOPS, 4)}
    if profile:
        kern, roof = mode_profile(eng, step, K, B3 * S3, S3, G, dims.layers)
        res["roofline"] = roof
        res["attention_us"] = kern.get("attention")
        res["kernels_avg_us"] = kern
        eng.set_streams(streams)
    return res


def second_mode_leg(args, mode, dims, weights, aids, alens, ids, lens, contract):
    """The default workload once more in the compute dtype that does NOT carry `value` (normally MV_F16, the `fast` object: one fp16
    sweep per GEMM): rate over the same K steps, per-class launch times, the dominant GEMM's roofline, its cfg-3 rate — and its
    trained-like logit error as measured in this run (`contract`), i.e. why it is not the headline."""
    B, S, G, K, W = args.batch, args.seq_len, args.anchors, args.steps, args.warmup
    res = {"compute_dtype": MODE_DTYPE[mode]}
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=max(B * S, 128 * 512), max_batch=max(B, 256),
                 max_anchors=max(G, 1024))
    eng.load_state_dict(weights, mode)
    eng.set_streams(args.streams)
    for s0 in range(0, G, 128):
        LA = int(alens[s0:s0 + 128].max())
        eng.anchor_append(aids[s0:s0 + 128, :LA], alens[s0:s0 + 128])
    eng.corpus_upload(ids, lens)
    n_batches = len(lens) // B

    def step(i):
        eng.corpus_run((i % n_batches) * B, B, B, keep_probs=False)

    for i in range(W):
        step(i)
    eng.sync()
    t0 = time.perf_counter()
    for i in range(K):
        step(W + i)
    eng.corpus_results(0, n_batches * B)
    dt = time.perf_counter() - t0
    res.update(value=round(K * B / dt, 2), unit="issue-reports/s", ms_per_step=round(dt / K * 1e3, 4), steps=K, warmup=W)
    fpi_exec = executed_flops_per_ir(S, G, dims.layers, cls_prune=os.environ.get("MEMVUL_CLS_PRUNE", "1") != "0")
    res["e2e_mfma_frac"] = round(res["value"] * fpi_exec / 1e12 / MFMA_PEAK_TFLOPS, 4)
    if not args.no_profile:
        res["kernels_avg_us"], res["roofline"] = mode_profile(eng, step, K, B * S, S, G, dims.layers)
        pmc, _ = load_pmc(mode) if (B, S) == (256, 256) else ({}, "")
        cls = pmc.get(res["roofline"]["kernel"], {})
        res["roofline"]["traffic"] = cls.get("traffic_bytes")
        res["roofline"].update({k: cls[k] for k in ("mfma_busy_frac", "effective_clock_ghz", "profiled_avg_us") if k in cls})
        eng.set_streams(args.streams)
    res["cfg3"] = {k: v for k, v in cfg3_leg(eng, dims, mode, min(K, 10), W, args.streams, profile=False).items() if k in ("value", "e2e_mfma_frac", "ms_per_step")}
    eng.close()
    if contract is not None:
        e = contract["logit_max_abs_err_trained_like"][mode]
        res["logit_max_abs_err_trained_like"] = e
        res["meets_contract"] = bool(e <= LOGIT_TOL)
    return res


if __name__ == "__main__":
    main()
