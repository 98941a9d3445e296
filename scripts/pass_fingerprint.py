"""The bits of an encoder pass, as hashes: what tests/test_pass_fingerprint_gpu.py holds a host-only rewrite of engine.hip (encode_dev, launch_attention and
what they call) to.  The oracle tolerances of the other GPU tests do not see a dropped row term or a stale GemmArgs field; an equal sha256 does.

A fixed matrix on a synthetic 2-layer model: ten handles (HANDLES: the compute dtypes, the forms and the switches that change what a launch is given) times
nine batches (BATCHES: every padded length, inputs narrower than their padded length, lengths on both sides of the [CLS]-row form's threshold).  Per handle and
batch: the sha256 of encode() (the pruned last layer), of every debug tap after debug_encode with 0, 1 and 2 layers (TAPS gives their order), and the launches
per kernel class of the encode(); on the default handle also the guarded forward and the sink census; per handle the saturation and concentration counters after
its runs.  The file keeps the first 12 hex digits of a sha256 (48 bits: plenty to tell "the same bits" from "other bits", a fifth of the bytes) and, of the two
libraries' kernel maps, one digest each.  Only binding.Engine calls that have not changed since the golden was recorded.

  python scripts/pass_fingerprint.py --out tests/golden/pass_fingerprints.json     (on an MI355X, at the commit the bits are to be pinned to)

A change that alters kernels (its build.kernel_fingerprints differ from the file's header) records the file again; the file's diff then shows which bits moved."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gpu_util as gu  # noqa: E402
import stage_kit as sk  # noqa: E402
from memvul_amd import binding, build  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pass_fingerprints.json")
DIMS = dict(layers=2, vocab_size=2048)
WEIGHTS = dict(qk_scale=3.0, match_scale=8.0)
# + the whole-pass [CLS]-row form at 384 (a pass at 384 whose shortest sequence has MEMVUL_CLS_ASIDE_MIN_LEN tokens); stage_kit has it at 192: (192, 130, (129, 130))
BATCHES = sk.BOUNDARY_BATCHES + ((384, 384, (257, 300, 384)),)
# name -> (compute dtype, form set after creation, switches read at mv_create, engine_for's gemm_tile)
HANDLES = {
    "precise": ("precise", None, {}, 0),
    "precise_safe": ("precise", "safe", {}, 0),
    "precise_cls_aside_0": ("precise", None, {"MEMVUL_CLS_ASIDE": "0"}, 0),
    "precise_qkv_aside_q": ("precise", None, {"MEMVUL_QKV_ASIDE": "q"}, 0),
    "precise_qkv_aside_qkv": ("precise", None, {"MEMVUL_QKV_ASIDE": "qkv"}, 0),
    "precise_cls_prune_0": ("precise", None, {"MEMVUL_CLS_PRUNE": "0"}, 0),
    "precise_short_vlo_0": ("precise", None, {"MEMVUL_SHORT_VLO": "0"}, 0),  # (a development switch: the development build)
    "f16": ("f16", None, {}, 0),  # the engine's own choice by pass size: the small-pass kernels at these sizes
    "f16_tile_512": ("f16", None, {}, 512),
    "f32": ("f32", None, {}, 0),
}
# a workspace of its own size (14 rows of 512 tokens fit): the handle is nobody else's, so what a tap holds where this pass wrote nothing is this run's too
ENGINE_KW = dict(max_tokens=8192, max_batch=16, max_anchors=8)


TAPS = [(n_layers, buf) for n_layers in (0, 1, 2) for buf in range(11)]  # debug_encode's layer count, debug_read's buffer: the order of a record's "taps"
TAPS_F32 = [(n_layers, buf) for n_layers in (0, 1, 2) for buf in (0, 10)]  # (an MV_F32 handle has no fp16 planes)


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:12]


def batch_ids(batch):
    return sk.boundary_ids(batch[1], batch[2], DIMS["vocab_size"], seed=len(batch[2]))


def open_handle(name):
    dtype, form, env, tile = HANDLES[name]
    eng = gu.engine_for(DIMS, WEIGHTS, gemm_tile=tile, env=env, compute_dtype=dtype, **ENGINE_KW)
    if form:
        eng.set_form(form)
    aids, alens = sk.boundary_ids(64, (5, 17, 40, 64), DIMS["vocab_size"], seed=77)
    eng.anchor_reset()
    eng.anchor_append(aids, alens)
    return eng


def close_handle(eng):
    """Out of gpu_util's cache as well: the next record of this handle starts on a fresh one."""
    for key in [k for k, e in gu._engines.items() if e is eng]:
        del gu._engines[key]
    eng.close()


def batch_record(eng, name, batch) -> dict:
    dtype = HANDLES[name][0]
    ids, lens = batch_ids(batch)
    rec = {}
    eng.profile_read()  # (drops what earlier calls left)
    eng.profile_enable(True)
    rec["encode"] = sha(eng.encode(ids, lens))
    rec["launches"] = [n for _, n in eng.profile_read().values()]  # (per kernel class, in the library's order: kernel_classes())
    eng.profile_enable(False)
    rec["taps"] = []
    for n_layers, buf in (TAPS_F32 if dtype == "f32" else TAPS):
        if buf == 0:
            eng.debug_encode(ids, lens, n_layers)
        try:
            rec["taps"].append(sha(eng.debug_read(buf)))
        except RuntimeError:  # (MV_F16 without its persistent path has no lo planes: the library says so)
            rec["taps"].append("-")
    if name == "precise":
        eng.set_form("guarded")
        out = eng.forward(ids, lens)
        rec["guarded_forward"] = sha(out["logits"], out["probs"], out["best"], out["best_idx"])
        rec["guarded_row_forms"] = "".join(f[0] for f in eng.last_row_forms())
        rec["guarded_form_stats"] = list(eng.form_stats())
        eng.set_form("default")
        eng.sink_census_enable(True)
        eng.encode(ids, lens)
        rec["sink_census"] = sha(*eng.sink_census_read(reset=True))
        eng.sink_census_enable(False)
    return rec


def handle_record(name) -> dict:
    eng = open_handle(name)
    try:
        rec = {sk.batch_id(b) + "_n%d" % len(b[2]): batch_record(eng, name, b) for b in BATCHES}
        if HANDLES[name][0] == "precise":
            rec["x8_saturation"] = eng.x8_saturation()
            m, over, total = eng.attention_concentration()
            rec["attention_concentration"] = [float(np.float32(m)).hex(), over, total]
    finally:
        close_handle(eng)
    return rec


def kernel_header() -> dict:
    """One digest per library over its build.kernel_fingerprints (scripts/kernel_fingerprints.py --against profiles/kernel_fingerprints*.json names the symbols)."""
    digest = lambda fp: hashlib.sha256(json.dumps(fp, sort_keys=True).encode()).hexdigest()  # noqa: E731
    return {"product": digest(build.kernel_fingerprints(build.LIB_PATH)), "development": digest(build.kernel_fingerprints(build.LIB_PATH_DEV))}


def kernel_classes() -> list:
    """The names of the kernel classes, in the order of a record's "launches"."""
    lib = binding.load_library()
    return [lib.mv_kernel_class_name(i).decode() for i in range(binding.NUM_KERNEL_CLASSES)]


def dump(doc: dict, path: str):
    """One line per (handle, batch): a moved hash is one changed line of the file's diff."""
    one = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))  # noqa: E731
    lines = ['{"commit":%s,' % one(doc["commit"]), '"kernel_fingerprints":%s,' % one(doc["kernel_fingerprints"]), '"kernel_classes":%s,' % one(doc["kernel_classes"]),
             '"handles":{']
    for i, (name, rec) in enumerate(sorted(doc["handles"].items())):
        lines.append('%s:{' % one(name))
        lines += ["%s:%s%s" % (one(k), one(v), "," if j + 1 < len(rec) else "") for j, (k, v) in enumerate(sorted(rec.items()))]
        lines.append("}" + ("," if i + 1 < len(doc["handles"]) else ""))
    with open(path, "w") as f:
        f.write("\n".join(lines + ["}}"]) + "\n")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", help="the commit the bits belong to (default: git rev-parse HEAD)")
    a = ap.parse_args(argv)
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    doc = {"commit": commit, "kernel_fingerprints": kernel_header(), "kernel_classes": kernel_classes(), "handles": {}}
    for name in HANDLES:
        doc["handles"][name] = handle_record(name)
        print(name, "done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dump(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
