"""What drives the indexes over a kept corpus (retrieve.ReportIndex, claims.ClaimIndex, bank.BankAudit, rank.RankIndex; kept_index.py is what they share below
this): KeptSweepState, the one owner of what ModelMemory knows about its last keeping sweep, and the command-line front of
``python -m memvul_amd.retrieve|claims|bank|rank``."""
from __future__ import annotations

import argparse
import contextlib
import json
from types import SimpleNamespace

import numpy as np

from .synth import KEY_MATCH_W

KINDS = ("reports", "claims", "bank", "ranking")


class KeptSweepState:
    """The last ``sweep_arrays(..., keep=True)`` of a ModelMemory and the indexes filled from it: ``rows`` = its ``(first, last)`` or None, ``matcher_weight`` =
    ``_projector.weight`` of the state dict or None, ``embed`` = the host copy of the kept embeddings or None, ``indexes`` = by kind, None until asked for.

    The host copy (2 KB per row): downloaded once, by the first index that is filled; dropped as soon as the report index and the claim index both exist, or with
    the state (``drop``).  The bank audit and the ranking index (rank.RankIndex) use the copy while it is there and never keep it alive or release it (filled after
    the other two, they download again and that copy goes by the same rule at once)."""

    def __init__(self, matcher_weight=None):
        self.matcher_weight = matcher_weight
        self.rows = self.embed = self._engine = None
        self.indexes = dict.fromkeys(KINDS)

    def require(self, who: str, first: int, last: int):
        if self.rows != (first, last):
            raise RuntimeError(f"{who}(): no kept sweep of these rows — call sweep_arrays(arrays, first, last, keep=True) first (the resident corpus keeps "
                               "its embeddings only when asked to)")

    def index(self, who: str, kind: str, index_class, engine, same_idx: int, index_factory=None, classes=None):
        """The index of ``kind`` over the kept sweep: filled through ``index_class.from_sweep`` at the first call, the same object afterwards."""
        if self.indexes[kind] is None:
            if self.matcher_weight is None:
                raise RuntimeError(f"{who}(): the state dict held no {KEY_MATCH_W}")
            self._engine = engine
            kw = {} if classes is None else {"classes": classes}
            self.indexes[kind] = index_class.from_sweep(self, self.matcher_weight, same_idx, index_factory=index_factory, **kw)
            if self.indexes["reports"] is not None and self.indexes["claims"] is not None:
                self.embed = None
        return self.indexes[kind]

    # -- what from_sweep asks of its ``engine`` argument
    device = property(lambda self: self._engine.device)
    P = property(lambda self: self._engine.P)

    def sweep_embeddings(self, first=0, count=None, chunk=65536):
        if self.embed is None:
            self.embed = self._engine.sweep_embeddings(0, None, chunk)
        return self.embed[first:None if count is None else first + count]

    def drop(self):
        """Close every index; forget the host copy and the rows (a new sweep or new weights replace what they were filled from)."""
        for kind in KINDS:
            index, self.indexes[kind] = self.indexes[kind], None
            if index is not None:
                index.close()
        self.rows = self.embed = self._engine = None


# ---- the command line of the three tools ---------------------------------------------------------------------------------------------------------------------------

def parser(prog: str, description: str) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument("--archive", required=True, help="model.tar.gz or its extracted directory")
    ap.add_argument("--golden", required=True, help="the golden anchor file ({cwe_id: description})")
    ap.add_argument("--input", required=True, help="the issue reports (a test_ / validation_ file of the reader)")
    return ap


def add_anchors(ap):
    ap.add_argument("--anchors", default=None, metavar="LABEL[,LABEL...]", help="only these anchors (default: all of the golden file)")


def add_output(ap, what: str):
    ap.add_argument("--out", default=None, help=f"write the {what} here instead of standard output")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--device", type=int, default=0)


def read_corpus(ap, args) -> SimpleNamespace:
    """What the arguments name, read: the state dict, the golden file's labels, the token ids of reports and anchors, the reports' urls and classes, and ``wanted``,
    the anchors ``--anchors`` selects (all of them where the tool has no such option)."""
    from . import archive as _archive
    from . import audit as _audit

    sd, config, same_idx = _audit._read_archive(args.archive)
    if config is None:
        ap.error("--archive must be an archive (config.json, vocabulary/, weights): the readers come from its config")
    reader = _archive._build_reader(config.get("validation_dataset_reader")) or _archive._build_reader(config.get("dataset_reader"))
    labels = list(reader.read_dataset(args.golden).keys())
    ids, lens, aids, alens = _audit._read_inputs(config, args.golden, args.input)
    arrays = reader.read_arrays(args.input)
    wanted = list(range(len(labels)))
    if getattr(args, "anchors", None) is not None:
        names = [a for a in args.anchors.split(",") if a]
        missing = [a for a in names if a not in labels]
        if missing:
            ap.error("--anchors: not in the golden file: " + ",".join(missing))
        wanted = [labels.index(a) for a in names]
    return SimpleNamespace(sd=sd, same_idx=same_idx, labels=labels, ids=ids, lens=lens, aids=aids, alens=alens, urls=arrays["urls"],
                           positive=np.asarray(arrays["same"], bool), wanted=wanted, wanted_labels=[labels[i] for i in wanted])


@contextlib.contextmanager
def filled_index(corpus, args, index_class, engine_factory=None, index_factory=None, classes=None):
    """``(index, vectors)``: an engine with the golden file's anchors, the reports swept and kept, ``index_class`` filled from that sweep, and the embeddings of the
    wanted anchors.  The index, then the engine, are closed on every way out."""
    from . import audit as _audit
    from . import binding

    c = corpus
    opts = dict(max_tokens=128 * 512, max_batch=max(512, args.batch), max_anchors=max(1024, len(c.alens)), same_idx=c.same_idx)
    opts.update(_audit._engine_dims(c.sd))
    eng = (engine_factory or binding.Engine)(args.device, **opts)
    try:
        eng.load_state_dict(c.sd)
        for i in range(len(c.alens)):  # (every anchor at its own length, the bank in the file's order)
            eng.anchor_append(np.ascontiguousarray(c.aids[i:i + 1, :max(int(c.alens[i]), 1)]), np.ascontiguousarray(c.alens[i:i + 1]))
        eng.bucketed_sweep(c.ids[:, :max(int(c.lens.max()), 1)], c.lens, args.batch, keep=True)
        kw = {} if classes is None else {"classes": classes}
        index = index_class.from_sweep(eng, np.asarray(c.sd[KEY_MATCH_W], np.float32), c.same_idx, index_factory=index_factory, **kw)
        try:
            yield index, np.ascontiguousarray(eng.anchor_get()[c.wanted], dtype=np.float32)
        finally:
            index.close()
    finally:
        eng.close()


def write_json(path, entries):
    """One JSON text per line, to ``path`` or to standard output."""
    lines = [json.dumps(e) for e in entries]
    if path:
        with open(path, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    else:
        print("\n".join(lines))
