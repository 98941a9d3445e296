"""Shared by the sink-census tests and scripts/make_sink_census_refs.py (test infrastructure — not the product path).

* ``cls_rows``: the float64 [CLS]-row probabilities of every (layer, sequence, head), obtained exactly as oracle/concentration.py obtains them — a recording
  format registered in ``precision_model.FORMATS`` for the length of one call, in the place of P's rounding.
* ``summarise``: per item the collision mass on the ordinary keys, the two largest ordinary shares and their token positions, and the third share.
* ``census_numpy``: a numpy RESTATEMENT of the kernel's bookkeeping (memvul_amd/csrc/sink_census.h) on given probabilities: the engine row order, rows >= 2,
  the map back to the token position, the lowest-position tie, the 16-token gate, the q20 rounding — with switches that break each of them
  (tests/test_sink_census_cpu.py shows that the checks below notice).
* ``bounds`` / ``check_census``: the checks of tests/test_sink_census_gpu.py on one call's histogram, from the reference alone."""
from __future__ import annotations

import numpy as np

from oracle import concentration as conc
from oracle import memvul_oracle as orc
from oracle import precision_model as pm

T = conc.THRESHOLD
MIN_LEN = conc.MIN_LEN
P_ROUNDING = 2.0 ** -10  # the monitor suite's relative part of the band (scripts/make_monitor_refs.py)
Q20 = float(1 << 20)
_SPY = "_census_row_spy"


def cls_rows(w, ids, lens, cfg=None, **encode_kw):
    """float64 [layers, B, heads, S]: the [CLS] row's attention probabilities in TOKEN order (cfg None: the exact forward; else the rounding model of a form)."""
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
        pm.encode(w, ids, conc.orc_mask(lens, ids.shape[1]), cfg, **encode_kw)
    finally:
        del pm.FORMATS[_SPY]
    assert len(rows) == L, (len(rows), L)
    p = np.stack(rows)
    return p / p.sum(-1, keepdims=True)


def summarise(p, lens):
    """Of p [layers, B, heads, S]: dict of [layers, B, heads] arrays — coll (sum of squares over positions 1 .. len - 2), pos1 / share1 (the largest ordinary
    share, ties to the lowest position), pos2 / share2 (the runner-up, at another position), share3."""
    L, B, H, _ = p.shape
    out = {k: np.zeros((L, B, H), np.int32 if k.startswith("pos") else np.float64) for k in ("coll", "pos1", "share1", "pos2", "share2", "share3")}
    for b, n in enumerate(np.asarray(lens)):
        n = int(n)
        if n < 5:
            continue
        o = p[:, b, :, 1:n - 1]
        out["coll"][:, b] = (o ** 2).sum(-1)
        order = np.argsort(-o, axis=-1, kind="stable")  # (stable: equal shares keep the lowest position first)
        top = np.take_along_axis(o, order[..., :3], -1)
        out["pos1"][:, b], out["pos2"][:, b] = order[..., 0] + 1, order[..., 1] + 1
        out["share1"][:, b], out["share2"][:, b], out["share3"][:, b] = top[..., 0], top[..., 1], top[..., 2]
    return out


def band(coll, delta_abs):
    return delta_abs + P_ROUNDING * coll


def census_numpy(p, ids, lens, vocab, drop_map=False, gate_gt=False, exclude_last_row=False, tie_high=False):
    """The kernel's bookkeeping on p [layers, B, heads, S] (token order): (items uint32 [vocab], share_q20 uint64 [vocab], by_head uint32 [layers, heads]).
    The switches are the four mistakes the CPU test plants."""
    L, B, H, _ = p.shape
    items, share, by_head = np.zeros(vocab, np.uint32), np.zeros(vocab, np.uint64), np.zeros((L, H), np.uint32)
    for b, n in enumerate(np.asarray(lens)):
        n = int(n)
        if (n <= MIN_LEN) if gate_gt else (n < MIN_LEN):
            continue
        pos_of_row = np.arange(n)  # engine row order: row 1 holds the last token, row len - 1 holds token 1 (embed_ln_kernel)
        pos_of_row[1], pos_of_row[n - 1] = n - 1, 1
        rows = np.array([r for r in range(n) if r != 0 and r != (n - 1 if exclude_last_row else 1)])
        for l in range(L):
            for h in range(H):
                e = p[l, b, h, pos_of_row[rows]].astype(np.float32)
                if not float((e.astype(np.float64) ** 2).sum()) > T:
                    continue
                pos = pos_of_row[rows]
                best = e.max()
                tied = pos[e == best]
                win = int(tied.max() if tie_high else tied.min())
                if drop_map:  # the winning ROW used as if it were a token position
                    win = int(rows[np.flatnonzero(pos == win)[0]])
                t = int(ids[b, win])
                items[t] += 1
                share[t] += np.uint64(int(np.rint(np.float32(best) * np.float32(Q20))))
                by_head[l, h] += 1
    return items, share, by_head


def bounds(ref, ids, lens, layers, vocab, delta_abs, m):
    """From one case's reference arrays (summarise, the first `layers` layers): what a census of that case may read.  Returns a dict:
    lo / hi [vocab] (certain items per token / + the uncertain ones that could fall to it), head_lo / head_hi [layers, heads], certain / uncertain counts,
    and per token the certain shares and the possible extra shares."""
    ids, lens = np.asarray(ids), np.asarray(lens)
    lo, hi = np.zeros(vocab, np.int64), np.zeros(vocab, np.int64)
    H = ref["coll"].shape[2]
    head_lo, head_hi = np.zeros((layers, H), np.int64), np.zeros((layers, H), np.int64)
    certain_shares, extra_shares = {}, {}
    n_uncertain = n_possible = 0
    for b, n in enumerate(lens):
        if int(n) < MIN_LEN:
            continue
        for l in range(layers):
            for h in range(H):
                c = float(ref["coll"][l, b, h])
                bd = band(c, delta_abs)
                if not c > T - bd:
                    continue
                n_possible += 1
                sure_over = c > T + bd
                s1, s2, s3 = (float(ref[k][l, b, h]) for k in ("share1", "share2", "share3"))
                assert s1 - s3 > m, ("three shares within the margin", l, b, h, s1, s2, s3)  # (the fixture script asserts it before it writes)
                t1, t2 = int(ids[b, int(ref["pos1"][l, b, h])]), int(ids[b, int(ref["pos2"][l, b, h])])
                sure_top = s1 - s2 >= m or t1 == t2  # (closer than m: uncertain; an exact tie at m = 0 is decided by the rule — the lowest position, pos1)
                head_hi[l, h] += 1
                head_lo[l, h] += sure_over
                if sure_over and sure_top:
                    lo[t1] += 1
                    hi[t1] += 1
                    certain_shares.setdefault(t1, []).append(s1)
                else:
                    n_uncertain += 1
                    for t, s in ((t1, s1),) if sure_top else ((t1, s1), (t2, s2)):
                        hi[t] += 1
                        extra_shares.setdefault(t, []).append(s)
    return dict(lo=lo, hi=hi, head_lo=head_lo, head_hi=head_hi, uncertain=n_uncertain, possible=n_possible, certain_shares=certain_shares, extra_shares=extra_shares)


def _mean_range(sure, extra):
    """The smallest and the largest mean of `sure` plus any subset of `extra` (at least one value in all)."""
    out = []
    for sign in (1.0, -1.0):
        vals, tot, cnt = sorted(sign * x for x in extra), sign * sum(sure), len(sure)
        for v in vals:  # ascending: a value lowers the mean exactly while it is below it
            if cnt == 0 or v < tot / cnt:
                tot, cnt = tot + v, cnt + 1
        out.append(sign * tot / cnt)
    return out[0], out[1]


def check_census(got, bd, m, what, controls=False):
    """The checks on one call's histogram `got` = (items, share_q20, by_head) against `bd` = bounds(...) (several cases: bounds added up by the caller).
    Returns (list of failures, largest |GPU mean share - reference mean share| over the tokens with certain items only)."""
    items, share, by_head = (np.asarray(a) for a in got)
    bad, gap = [], 0.0
    lo, hi = bd["lo"], bd["hi"]
    for t in np.flatnonzero((items < lo) | (items > hi)):
        bad.append(f"{what}: items[{t}] = {int(items[t])} outside [{int(lo[t])}, {int(hi[t])}]")
    if controls and items.any():
        bad.append(f"{what}: a control reads a non-zero histogram ({int(items.sum())} items)")
    nl = bd["head_lo"].shape[0]  # the monitored layers: the rows of by_head past them stay empty
    if by_head[nl:].any():
        bad.append(f"{what}: by_head counts in a layer that feeds no monitor")
    by_head = by_head[:nl]
    if ((by_head < bd["head_lo"]) | (by_head > bd["head_hi"])).any():
        bad.append(f"{what}: by_head outside its bounds at {np.argwhere((by_head < bd['head_lo']) | (by_head > bd['head_hi'])).tolist()[:6]}")
    if int(by_head.sum()) != int(items.sum()):
        bad.append(f"{what}: by_head sums to {int(by_head.sum())}, items to {int(items.sum())}")
    if not int(bd["head_lo"].sum()) <= int(items.sum()) <= int(bd["head_hi"].sum()):
        bad.append(f"{what}: {int(items.sum())} items outside the monitor's interval [{int(bd['head_lo'].sum())}, {int(bd['head_hi'].sum())}]")
    if share[items == 0].any():
        bad.append(f"{what}: share_q20 without items")
    for t in np.flatnonzero(items):
        mean = float(share[t]) / float(items[t]) / Q20
        sure, extra = bd["certain_shares"].get(int(t), []), bd["extra_shares"].get(int(t), [])
        if not sure and not extra:
            continue  # (already reported above)
        a, z = _mean_range(sure, extra)
        if not a - m <= mean <= z + m:
            bad.append(f"{what}: mean share of token {t} = {mean:.6f} outside [{a:.6f}, {z:.6f}] -+ {m:.2e}")
        if sure and not extra:
            gap = max(gap, abs(mean - a))
    return bad, gap


def add_bounds(a, b):
    """The bounds of two cases read in one histogram."""
    if a is None:
        return b
    out = {k: a[k] + b[k] for k in ("lo", "hi", "head_lo", "head_hi", "uncertain", "possible")}
    for k in ("certain_shares", "extra_shares"):
        out[k] = {t: a[k].get(t, []) + b[k].get(t, []) for t in set(a[k]) | set(b[k])}
    return out
