"""The contract audit: the logits of a 16-bit compute dtype (or form) against the library's own fp32 reference form, on the model and the data a user has.

Everything the library says about its precision rests on one comparison — engine logits against an fp32 evaluation of the same model.  The fp32 evaluation
used to exist only on the CPU (6 - 13 issue reports/s); compute dtype "f32" (include/memvul_hip.h MV_F32) runs the reference's arithmetic on the GPU, within
3e-5 of a float64 evaluation, so the comparison can be made wherever the library runs:

    python -m memvul_amd.audit --archive model.tar.gz --golden CWE_anchor_golden_project.json --input test_project.json --sample 2048 --forms precise,safe

prints one JSON line and exits 0 iff every audited form stays within the tolerance (1e-3 on the logits, model_memory.py:133-147).  `audit` is the same on
arrays; `compare` the statistics alone."""
from __future__ import annotations

import argparse
import json
import sys
import time
import warnings
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import binding

FORMS = ("precise", "safe", "guarded", "f16")  # what can be audited: the compute dtype names of binding.COMPUTE_DTYPES other than the reference form itself
PFX_BERT = "_text_field_embedder.token_embedder_tokens.transformer_model."


def _softmax2(logits: np.ndarray) -> np.ndarray:
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def compare(ref_logits, logits, tol: float = 1e-3, thres: float = 0.5, same_idx: int = 0) -> Dict[str, Any]:
    """|logits - ref_logits| of [B, G, 2] arrays, as a user reads it.  From the logits: `max`; per-row maxima (`row_max`, with `row_max_median` and
    `row_max_p90`); pooled `rms`, `p99`, `p999`; `rows_over` / `rows_over_idx` (rows whose maximum exceeds `tol`); `meets` = max <= tol.  From the
    probabilities (softmax over the last axis): `best_anchor_flips` = rows whose best anchor (first argmax of P(same) over the anchors) differs, and
    `threshold_crossings` = rows whose best P(same) lies on the other side of `thres` — what a prediction file finally shows."""
    ref = np.asarray(ref_logits, np.float64)
    got = np.asarray(logits, np.float64)
    if ref.shape != got.shape or ref.ndim != 3 or ref.shape[-1] != 2:
        raise ValueError(f"compare: expected two [B, G, 2] arrays, got {ref.shape} and {got.shape}")
    B = ref.shape[0]
    d = np.abs(got - ref)
    row_max = d.reshape(B, -1).max(1) if d.size else np.zeros(B)
    over = np.flatnonzero(row_max > tol)
    ps_ref, ps = _softmax2(ref)[:, :, same_idx], _softmax2(got)[:, :, same_idx]
    if d.size:
        b_ref, b = ps_ref.argmax(1), ps.argmax(1)
        top_ref, top = ps_ref[np.arange(B), b_ref], ps[np.arange(B), b]
        flips, cross = int((b_ref != b).sum()), int(((top_ref >= thres) != (top >= thres)).sum())
    else:
        flips = cross = 0
    q = (lambda v, p: float(np.percentile(v, p))) if d.size else (lambda v, p: 0.0)
    mx = float(d.max()) if d.size else 0.0
    return {"rows": int(B), "anchors": int(ref.shape[1]), "tol": float(tol), "max": mx, "meets": bool(mx <= tol),
            "row_max": [float(x) for x in row_max], "row_max_median": q(row_max, 50), "row_max_p90": q(row_max, 90),
            "rms": float(np.sqrt((d * d).mean())) if d.size else 0.0, "p99": q(d, 99), "p999": q(d, 99.9),
            "rows_over": int(over.size), "rows_over_idx": [int(i) for i in over],
            "thres": float(thres), "best_anchor_flips": flips, "threshold_crossings": cross}


def sample_rows(lens, n: Optional[int]) -> np.ndarray:
    """`n` row indices evenly spaced over the length-sorted input (stable sort, so the choice is deterministic), ascending: every length bucket the input
    has is represented in proportion.  None, or n >= the row count: every row."""
    lens = np.asarray(lens)
    if n is None or n >= len(lens):
        return np.arange(len(lens))
    if n <= 0:
        raise ValueError("sample must be positive")
    order = np.argsort(lens, kind="stable")
    pick = np.unique(np.round(np.linspace(0, len(lens) - 1, n)).astype(np.int64))
    return np.sort(order[pick])


def _padded_len(n: int) -> int:  # encoder_pass.h padded_len
    n = max(int(n), 1)
    return (n + 63) // 64 * 64 if n <= 256 else (n + 127) // 128 * 128


def _engine_dims(sd: Dict[str, np.ndarray]) -> Dict[str, int]:
    layers = 0
    while (PFX_BERT + f"encoder.layer.{layers}.attention.self.query.weight") in sd:
        layers += 1
    return dict(vocab_size=int(sd[PFX_BERT + "embeddings.word_embeddings.weight"].shape[0]), layers=layers,
                max_pos=min(512, int(sd[PFX_BERT + "embeddings.position_embeddings.weight"].shape[0])),
                type_vocab=int(sd[PFX_BERT + "embeddings.token_type_embeddings.weight"].shape[0]),
                proj_dim=512 if "_projector_single._linear_layers.0.weight" in sd else 768)


CENSUS_TOP = 10  # tokens the --census list names per form


def _sink_tokens(eng, ids, lens) -> list:
    """The sink census of the rows just scored, most flagged items first; `sequences_with_token` = the share of those rows that contain the token — the f to put
    into the guarded form's 1 + 1.34 f if that token is what its heads sit on (include/memvul_hip.h mv_set_form)."""
    rows = eng.sink_census(top=CENSUS_TOP)["tokens"]
    valid = np.arange(ids.shape[1])[None, :] < np.asarray(lens)[:, None]
    for r in rows:
        r["sequences_with_token"] = float(((ids == r["token_id"]) & valid).any(1).mean()) if len(lens) else 0.0
    return rows


def _score(engine_factory, sd, compute: str, ids, lens, anchor_ids, anchor_lens, batch: int, opts: Dict[str, Any], census: bool = False,
           sink_tokens: Optional[Sequence[int]] = None) -> Dict[str, Any]:
    """One engine of compute dtype `compute`: the anchors appended in order — consecutive anchors of one padded length per call, cut to the longest of them,
    so every anchor runs at the padded length of its own token count — the rows scored through forward_by_length in batches; then closed.  sink_tokens: the
    sink-token list the engine gets before anything is encoded (the guarded form's: audit() hands it to no other)."""
    eng = engine_factory(0 if "device" not in opts else opts["device"], **{k: v for k, v in opts.items() if k != "device"})
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the monitors are reported below, as numbers
            eng.load_state_dict(sd, compute)
            if sink_tokens is not None:
                eng.set_sink_tokens(list(sink_tokens))
            eng.anchor_reset()
            g0, G = 0, len(anchor_lens)
            while g0 < G:
                g1 = g0 + 1
                while g1 < G and g1 - g0 < 128 and _padded_len(anchor_lens[g1]) == _padded_len(anchor_lens[g0]):
                    g1 += 1
                L = max(int(np.max(anchor_lens[g0:g1])), 1)
                eng.anchor_append(np.ascontiguousarray(anchor_ids[g0:g1, :L]), np.ascontiguousarray(anchor_lens[g0:g1]))
                g0 = g1
            census = census and compute in ("precise", "safe", "guarded") and hasattr(eng, "sink_census_enable")  # (MV_F16X8 only; after the anchors: the issue reports alone)
            if census:
                eng.sink_census_enable(True)
            logits = np.empty((len(lens), G, 2), np.float32)
            t0 = time.perf_counter()
            for s0 in range(0, len(lens), batch):
                part = lens[s0:s0 + batch]
                L = max(int(part.max()), 1)
                out = eng.forward_by_length(np.ascontiguousarray(ids[s0:s0 + batch, :L]), np.ascontiguousarray(part), want_logits=True, want_probs=False)
                logits[s0:s0 + batch] = out["logits"]
            dt = time.perf_counter() - t0
            mon: Dict[str, Any] = {}
            if hasattr(eng, "attention_concentration"):
                mx, over, total = eng.attention_concentration()
                mon.update(max_collision=float(mx), items_over=int(over), items_total=int(total))
            if hasattr(eng, "x8_saturation"):
                mon["x8_saturation"] = int(eng.x8_saturation())
            if compute == "guarded" and hasattr(eng, "form_stats"):
                seqs, resc = eng.form_stats()
                mon.update(guarded_sequences=int(seqs), guarded_rescored=int(resc))
                if sink_tokens is not None:
                    mon["guarded_routed"] = int(eng.route_stats())
            sink_tokens = _sink_tokens(eng, ids, lens) if census else None
        return {"logits": logits, "monitors": mon, "reports_per_s": float(len(lens) / dt) if dt > 0 else 0.0, "sink_tokens": sink_tokens}
    finally:
        eng.close()


def audit(state_dict_or_archive, ids, lens, anchor_ids, anchor_lens, forms: Sequence[str] = ("precise",), sample: Optional[int] = None,
          engine_factory=binding.Engine, tol: float = 1e-3, thres: float = 0.5, same_idx: int = 0, batch: int = 512,
          engine_options: Optional[Dict[str, Any]] = None, keep_logits: bool = False, census: bool = False,
          sink_tokens: Optional[Sequence[int]] = None) -> Dict[str, Any]:
    """The audit on arrays.  `state_dict_or_archive`: the reference's state dict (name -> array) or the path of an archive (model.tar.gz, its directory, or a
    weights file archive.read_state_dict reads).  ids [N, S] zero-padded / lens [N]: the issue reports; anchor_ids / anchor_lens: the golden anchors.
    Scores `sample` rows (sample_rows; None = all) on an "f32" engine — the reference — then on one engine per name in `forms` ("precise", "safe",
    "guarded", "f16"), one engine alive at a time, and returns {"rows", "reference": {reports_per_s}, "forms": {name: compare(...) + monitors +
    reports_per_s}, "meets": every form within tol}.  engine_factory(device, **options) builds the engines (the CPU suite passes an oracle-backed stand-in).
    keep_logits: also return the logits ("reference"/"forms"[name]["logits"]: arrays, not JSON).  census: every MV_F16X8 form also gets "sink_tokens" — the
    sink census of its scored rows (binding.Engine.sink_census) with, per token, the share of those rows that contain it; nothing else changes.
    sink_tokens: the sink-token list (binding.Engine.set_sink_tokens) of the audited "guarded" form — an error without "guarded" among `forms`; that form's object
    gains "sink_token_list", "rescored_share" and "routed_share" (of the sequences it encoded, anchors included), and with `census` its "sink_tokens" then shows
    what the list does NOT cover: a routed sequence feeds no census."""
    for f in forms:
        if f not in FORMS:
            raise ValueError(f"audit: unknown form {f!r}: expected a subset of {FORMS}")
    if sink_tokens is not None:
        sink_tokens = binding._sink_token_list(sink_tokens)
        if "guarded" not in forms:
            raise ValueError("audit: sink_tokens is acted on in the guarded form only: add \"guarded\" to the forms")
    if isinstance(state_dict_or_archive, str):
        sd, _, same_idx = _read_archive(state_dict_or_archive)  # (the archive's own index of "same"; a bare weights file: 0)
    else:
        sd = {k: np.asarray(v) for k, v in state_dict_or_archive.items()}
    ids, lens = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lens, np.int32)
    anchor_ids, anchor_lens = np.ascontiguousarray(anchor_ids, np.int32), np.ascontiguousarray(anchor_lens, np.int32)
    rows = sample_rows(lens, sample)
    ids, lens = ids[rows], lens[rows]
    opts = dict(max_tokens=128 * 512, max_batch=max(512, batch), max_anchors=max(1024, len(anchor_lens)), same_idx=same_idx)
    opts.update(_engine_dims(sd))
    opts.update(engine_options or {})
    ref = _score(engine_factory, sd, "f32", ids, lens, anchor_ids, anchor_lens, batch, opts)
    res: Dict[str, Any] = {"rows": [int(r) for r in rows], "anchors": int(len(anchor_lens)), "tol": float(tol), "thres": float(thres),
                           "reference": {"compute": "f32", "reports_per_s": ref["reports_per_s"]}, "forms": {}}
    if keep_logits:
        res["reference"]["logits"] = ref["logits"]
    for f in forms:
        got = _score(engine_factory, sd, f, ids, lens, anchor_ids, anchor_lens, batch, opts, census, sink_tokens if f == "guarded" else None)
        r = compare(ref["logits"], got["logits"], tol=tol, thres=thres, same_idx=same_idx)
        r["rows_over_idx"] = [int(rows[i]) for i in r["rows_over_idx"]]  # in the caller's numbering
        r["monitors"], r["reports_per_s"] = got["monitors"], got["reports_per_s"]
        if got["sink_tokens"] is not None:
            r["sink_tokens"] = got["sink_tokens"]
        if f == "guarded" and sink_tokens is not None:
            seqs = max(int(got["monitors"].get("guarded_sequences", 0)), 1)
            r["sink_token_list"] = [int(t) for t in sink_tokens]
            r["rescored_share"] = int(got["monitors"].get("guarded_rescored", 0)) / seqs
            r["routed_share"] = int(got["monitors"].get("guarded_routed", 0)) / seqs
        if keep_logits:
            r["logits"] = got["logits"]
        res["forms"][f] = r
    res["meets"] = all(r["meets"] for r in res["forms"].values())
    return res


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------

def _read_archive(path: str):
    """(state dict, config or None, index of "same") of an archive file / directory, or of a bare weights file."""
    import os
    import tarfile
    import tempfile

    from . import archive as _archive
    from . import params as _params
    from .registry import Vocabulary

    if os.path.isfile(path) and not tarfile.is_tarfile(path):
        return _archive.read_state_dict(path), None, 0
    tmp = None
    root = path
    if os.path.isfile(path):
        tmp = tempfile.TemporaryDirectory(prefix="memvul_archive_")
        with tarfile.open(path, "r:*") as tf:
            tf.extractall(tmp.name, filter="data")
        root = tmp.name
    try:
        config = _params.load_config(os.path.join(root, "config.json"))
        vocab = Vocabulary.from_files(os.path.join(root, "vocabulary"))
        same_idx = vocab.get_token_index("same", namespace=config["model"].get("label_namespace", "labels"))
        for cand in ("weights.th", "weights.safetensors", "weights.npz"):
            if os.path.exists(os.path.join(root, cand)):
                return _archive.read_state_dict(os.path.join(root, cand)), config, int(same_idx)
        raise FileNotFoundError(f"no weights.th in {path}")
    finally:
        if tmp is not None:
            tmp.cleanup()


def _read_inputs(config, golden_path: str, input_path: str):
    """The golden anchors and the issue reports of predict_memory's files as id arrays, through the archive's (validation) dataset reader: the anchors in file
    order (reader_memory.py:73-79), the issue reports in the reader's order (read_arrays)."""
    from . import archive as _archive

    reader = _archive._build_reader(config.get("validation_dataset_reader")) or _archive._build_reader(config.get("dataset_reader"))
    golden = reader.read_dataset(golden_path)
    rows = [[int(t.text_id) for t in group[0]["description"]] for group in golden.values()]
    alens = np.array([len(r) for r in rows], np.int32)
    aids = np.zeros((len(rows), int(alens.max())), np.int32)
    for i, r in enumerate(rows):
        aids[i, :len(r)] = r
    arr = reader.read_arrays(input_path)
    return arr["ids"], arr["lens"], aids, alens


def main(argv=None, engine_factory=binding.Engine) -> int:
    ap = argparse.ArgumentParser(prog="python -m memvul_amd.audit", description="Audit the logit contract of a checkpoint on a corpus against the fp32 reference form.")
    ap.add_argument("--archive", required=True, help="model.tar.gz or its extracted directory")
    ap.add_argument("--golden", required=True, help="the golden anchor file ({cwe_id: description})")
    ap.add_argument("--input", required=True, help="the issue reports (a test_ / validation_ file of the reader)")
    ap.add_argument("--sample", type=int, default=None, help="rows to score, evenly spaced over the length-sorted input (default: all)")
    ap.add_argument("--forms", default="precise", help="comma-separated subset of " + ",".join(FORMS))
    ap.add_argument("--thres", type=float, default=0.5, help="threshold on the best P(same) whose crossings are counted")
    ap.add_argument("--tol", type=float, default=1e-3, help="tolerance on the logits")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--census", action="store_true", help="add the sink census of every MV_F16X8 form: which tokens its flagged heads sit on (sink_tokens)")
    ap.add_argument("--sink-tokens", default=None, metavar="ID[,ID...]", help="the sink-token list of the audited guarded form (needs guarded among --forms): its "
                    "object gains routed_share; with --census its sink_tokens shows what the list does not cover")
    args = ap.parse_args(argv)
    forms = tuple(f for f in args.forms.split(",") if f)
    sink_tokens = None
    if args.sink_tokens is not None:
        try:
            sink_tokens = binding.parse_sink_tokens(args.sink_tokens)
        except ValueError as e:
            ap.error(str(e).replace("MEMVUL_SINK_TOKENS=", "--sink-tokens "))
        if "guarded" not in forms:
            ap.error("--sink-tokens is acted on in the guarded form only: add guarded to --forms")
    sd, config, same_idx = _read_archive(args.archive)
    if config is None:
        ap.error("--archive must be an archive (config.json, vocabulary/, weights): the readers come from its config")
    ids, lens, aids, alens = _read_inputs(config, args.golden, args.input)
    res = audit(sd, ids, lens, aids, alens, forms=forms, sample=args.sample, engine_factory=engine_factory,
                tol=args.tol, thres=args.thres, same_idx=same_idx, engine_options={"device": args.device}, census=args.census, sink_tokens=sink_tokens)
    for r in res["forms"].values():
        r.pop("row_max", None)  # one line a person can read: the per-row maxima stay with audit()
    print(json.dumps(res))
    return 0 if res["meets"] else 1


if __name__ == "__main__":
    sys.exit(main())
