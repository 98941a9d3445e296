"""Per-anchor retrieval over a kept corpus: which issue reports does an anchor attract?  ctypes binding of libmemvul_retrieve.so (include/memvul_retrieve.h;
kernels: csrc/report_topk.h) and its command line.

The engine answers "which anchors fit this report"; a ReportIndex answers the other direction: for every query vector — an anchor of the bank, or
``engine.encode(...)`` of a fresh CVE description — the k rows of the corpus with the highest P(same), ranked ``(P descending, row ascending)`` on the GPU.  P(same) of
a pair is bit for bit what the engine's matcher gives for it.  As everywhere in this package there is no CPU fallback.

  python -m memvul_amd.retrieve --archive A --golden G --input T --k 20 [--anchors CWE-79,CWE-89] [--out FILE]

writes one JSON line per anchor: {"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]}."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_retrieve.so")

MAX_K, MAX_QUERIES, MAX_ROWS, MAX_PSAME = 64, 4096, 2 ** 31 - 2, 2 ** 28  # include/memvul_retrieve.h
KEY_MATCH_W = "_projector.weight"

_f32p, _vp = C.POINTER(C.c_float), C.c_void_p
_SIGNATURES = {
    "mvr_create": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "mvr_destroy": (None, [_vp]),
    "mvr_last_error": (C.c_char_p, [_vp]),
    "mvr_add": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvr_reset": (C.c_int, [_vp]),
    "mvr_count": (C.c_int64, [_vp]),
    "mvr_query": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, _vp]),
    "mvr_psame": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, _vp]),
    "mvr_kernel_ms": (C.c_int, [_vp, _f32p]),
    "mvr_test_plan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
}
RETRIEVE_SYMBOLS = list(_SIGNATURES)

_libs = {}


def load_library(path: Optional[str] = None):
    """dlopen libmemvul_retrieve.so and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"libmemvul_retrieve.so not found at {path}: build it with `python -m memvul_amd.build` (hipcc --offload-arch=gfx950); "
                           "per-anchor retrieval has no CPU fallback")
    try:
        lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    _libs[path] = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _check_array(a, what: str, width: int) -> np.ndarray:
    """float32, C-contiguous, [n, width]: checked, never converted (a silent copy of a 2.5 GB corpus is not a service)."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{what}: a numpy array, not {type(a).__name__}")
    if a.dtype != np.float32:
        raise TypeError(f"{what}: float32, not {a.dtype}")
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: shape [n, {width}], not {list(a.shape)}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{what}: must be C-contiguous")
    return a


def _int(x, what: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{what}: an integer, not {type(x).__name__}")
    return int(x)


class ReportIndex:
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim]."""

    def __init__(self, device: int, proj_dim: int, matcher_weight, same_idx: int, lib=None):
        self._h = None
        device, proj_dim, same_idx = _int(device, "device"), _int(proj_dim, "proj_dim"), _int(same_idx, "same_idx")
        if proj_dim not in (512, 768):
            raise ValueError(f"proj_dim = {proj_dim}: the matcher runs on 512 or 768 features")
        if same_idx not in (0, 1):
            raise ValueError(f"same_idx = {same_idx}: 0 or 1")
        if device < 0:
            raise ValueError(f"device = {device}")
        w = np.asarray(matcher_weight)
        if w.dtype != np.float32 or w.shape != (2, 3 * proj_dim):
            raise ValueError(f"matcher_weight: float32 [2, {3 * proj_dim}], not {w.dtype} {list(w.shape)}")
        w = np.ascontiguousarray(w)
        self._lib = lib if lib is not None else load_library()
        self.P, self.same_idx, self.device = proj_dim, same_idx, device
        h = C.c_void_p()
        rc = self._lib.mvr_create(device, proj_dim, _ptr(w), same_idx, C.byref(h))
        if rc != 0:
            msg = self._lib.mvr_last_error(None)
            raise RuntimeError(f"mvr_create failed ({rc}): {msg.decode() if msg else ''}")
        self._h = h

    # -- plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.mvr_last_error(self._h)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _handle(self):
        if self._h is None:
            raise RuntimeError("the ReportIndex is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mvr_destroy(self._h)
        self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- the rows
    def add(self, embed: np.ndarray):
        """Append rows: float32 [n, proj_dim], C-contiguous.  Rows are numbered in order of arrival."""
        h = self._handle()
        embed = _check_array(embed, "embed", self.P)
        if len(self) + embed.shape[0] > MAX_ROWS:
            raise ValueError("the index would hold more than 2^31 - 2 rows")
        self._check(self._lib.mvr_add(h, _ptr(embed), embed.shape[0]), "mvr_add")

    def reset(self):
        """Forget the rows, keep the weights."""
        self._check(self._lib.mvr_reset(self._handle()), "mvr_reset")

    def __len__(self) -> int:
        return int(self._lib.mvr_count(self._handle()))

    def _range(self, first, count):
        n = len(self)
        first = _int(first, "first")
        count = n - first if count is None else _int(count, "count")
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"rows [{first}, {first} + {count}) are not within the {n} rows of the index")
        return first, count

    def _vectors(self, vectors) -> np.ndarray:
        vectors = _check_array(vectors, "vectors", self.P)
        if not 1 <= vectors.shape[0] <= MAX_QUERIES:
            raise ValueError(f"{vectors.shape[0]} query vectors: 1 <= Q <= {MAX_QUERIES}")
        return vectors

    # -- the questions
    def query(self, vectors: np.ndarray, k: int, first: int = 0, count: Optional[int] = None):
        """For each of the Q vectors the k best rows among [first, first + count): ``(p float32 [Q, k], rows int64 [Q, k])``, ranked (P(same) descending, row
        ascending; a NaN ranks first).  Slots beyond the rows in range hold p = -1, row = -1."""
        h = self._handle()
        vectors = self._vectors(vectors)
        k = _int(k, "k")
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k = {k}: 1 <= k <= {MAX_K}")
        first, count = self._range(first, count)
        Q = vectors.shape[0]
        p, rows = np.empty((Q, k), np.float32), np.empty((Q, k), np.int64)
        self._check(self._lib.mvr_query(h, _ptr(vectors), Q, k, first, count, _ptr(p), _ptr(rows)), "mvr_query")
        return p, rows

    def psame(self, vectors: np.ndarray, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """P(same) float32 [count, Q] of rows [first, first + count) against every vector (count * Q <= 2^28 per call)."""
        h = self._handle()
        vectors = self._vectors(vectors)
        first, count = self._range(first, count)
        Q = vectors.shape[0]
        if count * Q > MAX_PSAME:
            raise ValueError(f"count * Q = {count * Q}: at most 2^28 values per call")
        p = np.empty((count, Q), np.float32)
        self._check(self._lib.mvr_psame(h, _ptr(vectors), Q, first, count, _ptr(p)), "mvr_psame")
        return p

    def kernel_ms(self) -> float:
        """HIP-event time of the last query's launches, in milliseconds."""
        ms = C.c_float()
        self._check(self._lib.mvr_kernel_ms(self._handle(), C.byref(ms)), "mvr_kernel_ms")
        return float(ms.value)

    def test_plan(self, block_rows: int = 0, fan_in: int = 0, anchor_group: int = 0):
        """Tests only: rows per block, lists per merge launch, query vectors per group (0 = the library's own choice).  No result depends on them."""
        self._check(self._lib.mvr_test_plan(self._handle(), int(block_rows), int(fan_in), int(anchor_group)), "mvr_test_plan")

    @classmethod
    def from_sweep(cls, engine, matcher_weight, same_idx: int, chunk: int = 65536, index_factory=None):
        """An index over the kept embeddings of the engine's last ``bucketed_sweep(..., keep=True)``, in the ORIGINAL row order, downloaded ``chunk`` rows at a time
        (one download and one upload per kept sweep: the engine's ABI has no entry that hands its resident embeddings over on the device)."""
        chunk = _int(chunk, "chunk")
        if chunk < 1:
            raise ValueError(f"chunk = {chunk}")
        embed = engine.sweep_embeddings(0, None, chunk)  # (raises unless the last sweep kept its embeddings; host memory: the whole corpus once, n * P * 4 bytes)
        index = (index_factory or cls)(engine.device, engine.P, matcher_weight, same_idx)
        try:
            for s0 in range(0, embed.shape[0], chunk):
                index.add(np.ascontiguousarray(embed[s0:s0 + chunk], dtype=np.float32))
        except Exception:
            index.close()
            raise
        return index


def format_reports(labels, urls, p: np.ndarray, rows: np.ndarray, first: int = 0) -> list:
    """One entry per query vector: {"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]} (exhausted slots left out).  rows: row numbers of the index;
    ``first``: the row of ``urls`` that row 0 of the index is."""
    out = []
    for g, label in enumerate(labels):
        reports = [{"Issue_Url": urls[first + int(r)], "row": first + int(r), "prob": float(pp)} for pp, r in zip(p[g], rows[g]) if r >= 0]
        out.append({"anchor": label, "reports": reports})
    return out


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None, engine_factory=None, index_factory=None) -> int:
    from . import audit as _audit
    from . import binding

    ap = argparse.ArgumentParser(prog="python -m memvul_amd.retrieve", description="For every anchor of the golden file: the k issue reports it attracts most.")
    ap.add_argument("--archive", required=True, help="model.tar.gz or its extracted directory")
    ap.add_argument("--golden", required=True, help="the golden anchor file ({cwe_id: description})")
    ap.add_argument("--input", required=True, help="the issue reports (a test_ / validation_ file of the reader)")
    ap.add_argument("--k", type=int, default=20, help="reports per anchor (1 .. 64)")
    ap.add_argument("--anchors", default=None, metavar="LABEL[,LABEL...]", help="only these anchors (default: all of the golden file)")
    ap.add_argument("--out", default=None, help="write the JSON lines here instead of standard output")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if not 1 <= args.k <= MAX_K:
        ap.error(f"--k {args.k}: 1 .. {MAX_K}")
    sd, config, same_idx = _audit._read_archive(args.archive)
    if config is None:
        ap.error("--archive must be an archive (config.json, vocabulary/, weights): the readers come from its config")
    from . import archive as _archive

    reader = _archive._build_reader(config.get("validation_dataset_reader")) or _archive._build_reader(config.get("dataset_reader"))
    labels = list(reader.read_dataset(args.golden).keys())
    ids, lens, aids, alens = _audit._read_inputs(config, args.golden, args.input)
    urls = reader.read_arrays(args.input)["urls"]
    wanted = list(range(len(labels)))
    if args.anchors is not None:
        names = [a for a in args.anchors.split(",") if a]
        missing = [a for a in names if a not in labels]
        if missing:
            ap.error("--anchors: not in the golden file: " + ",".join(missing))
        wanted = [labels.index(a) for a in names]
    opts = dict(max_tokens=128 * 512, max_batch=max(512, args.batch), max_anchors=max(1024, len(alens)), same_idx=same_idx)
    opts.update(_audit._engine_dims(sd))
    eng = (engine_factory or binding.Engine)(args.device, **opts)
    try:
        eng.load_state_dict(sd)
        for i in range(len(alens)):  # (every anchor at its own length, the bank in the file's order)
            eng.anchor_append(np.ascontiguousarray(aids[i:i + 1, :max(int(alens[i]), 1)]), np.ascontiguousarray(alens[i:i + 1]))
        eng.bucketed_sweep(ids[:, :max(int(lens.max()), 1)], lens, args.batch, keep=True)
        index = ReportIndex.from_sweep(eng, np.asarray(sd[KEY_MATCH_W], np.float32), same_idx, index_factory=index_factory)
        try:
            v = np.ascontiguousarray(eng.anchor_get()[wanted], dtype=np.float32)
            p, rows = index.query(v, min(args.k, MAX_K))
        finally:
            index.close()
    finally:
        eng.close()
    lines = [json.dumps(e) for e in format_reports([labels[i] for i in wanted], urls, p, rows)]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    else:
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
