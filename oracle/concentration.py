"""CPU ORACLE (test infrastructure — NOT the product path): the float64 reference of the attention kernel's concentration monitor.

The monitor (memvul_amd/csrc/attention_v2.h, AttnArgs::conc / AttnArgs::seq_over; include/memvul_hip.h mv_attention_concentration) keeps, per (layer, sequence,
head) item, the COLLISION MASS of the [CLS] row on the ordinary keys: sum p[CLS row][j]^2 over every key j except the sequence's first ([CLS]) and last ([SEP])
token.  Here the same number comes out of oracle/precision_model.py's forward: a recording format stands in the place of P's rounding for the length of one
call, so the probabilities are read exactly where the engine rounds them (after the exp, before P V), in the sequence's own token order."""
from __future__ import annotations

import numpy as np

from . import memvul_oracle as orc
from . import precision_model as pm

THRESHOLD = 0.25  # MV_SINK_COLLISION (memvul_amd/csrc/attention.h)
MIN_LEN = 16      # sequences of fewer tokens are not looked at (attention_v2.h, batch_flow.h guard_flagged)
GUARD_SHARE = 0.02  # kGuardShare (batch_flow.h)
_SPY = "_cls_row_spy"


def cls_collision(w, ids, lens, cfg=None, forward=None, with_output=False, **encode_kw):
    """float64 [layers, B, heads]: the collision mass of the [CLS] row of every (layer, sequence, head) over keys 1 .. len - 2.

    ``cfg`` None: the exact forward; a ``precision_model.engine_formats(...)`` configuration: the rounding model of a form (its ``p`` knob is replaced by the
    recording format: P itself is read unrounded).  ``encode_kw``: keyword arguments of ``precision_model.encode`` (e.g. ``**precision_model.SHIPPED_KW``).
    ``forward``: the function of precision_model that runs (``encode`` unless given, e.g. ``instance_forward``); ``with_output``: return (collision, its result)."""
    ids, lens = np.asarray(ids), np.asarray(lens)
    L = orc.n_layers(w)
    cfg = pm.engine_formats(L, "exact") if cfg is None else {k: list(v) for k, v in cfg.items()}
    cfg["p"] = [_SPY] * L
    rows = []

    def spy(e):  # e [B, heads, S, S]: exp(score - row max), unnormalised
        rows.append(np.array(e[:, :, 0, :], np.float64))
        return e

    pm.FORMATS[_SPY] = spy
    try:
        out = (forward or pm.encode)(w, ids, orc_mask(lens, ids.shape[1]), cfg, **encode_kw)
    finally:
        del pm.FORMATS[_SPY]
    assert len(rows) == L, (len(rows), L)
    coll = np.zeros((L, len(lens), rows[0].shape[1]))
    for l, e in enumerate(rows):
        p = e / e.sum(-1, keepdims=True)  # [B, heads, S]
        for b, n in enumerate(lens):
            coll[l, b] = (p[b, :, 1:int(n) - 1] ** 2).sum(-1)
    return (coll, out) if with_output else coll


def orc_mask(lens, S):
    return np.arange(S)[None, :] < np.asarray(lens)[:, None]


def items_total(lens, monitored_layers, heads=12):
    """Items the monitor looks at per sequence: every head of every monitored layer, for sequences of at least MIN_LEN tokens."""
    return np.where(np.asarray(lens) >= MIN_LEN, heads * monitored_layers, 0)


def rule(over, lens, monitored_layers, heads=12):
    """The per-sequence rule of the guarded form (batch_flow.h guard_flagged): more than GUARD_SHARE of the sequence's own items over THRESHOLD."""
    return np.asarray(over) > GUARD_SHARE * items_total(lens, monitored_layers, heads)
