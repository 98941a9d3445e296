// Part of engine.hip: the one batch flow of the host-buffer entry points — the planner (plan_batch, cut_passes), the pass loop (run_passes), the row scatter,
// the guarded form's rescoring of a host batch (rescore_rows) with the sink-token routing (scan_routed, split_plan), and enqueue_batch / collect_batch.

namespace {

// largest batch one encoder pass can take at padded length Sp
int max_rows_for(mv_handle* h, int S_in) {
  const int Sp = padded_len(S_in);
  int64_t r = (h->cap_tokens - 256) / Sp;
  if (r > h->cfg.max_batch) r = h->cfg.max_batch;
  return (int)r;
}

// ---- the one planner, the one pass cutter, the one pass loop, the one row scatter ---------------------------------------------------------------------------------
// cut_passes: appends to pl the passes of its rows [start, end) at `width` tokens per row: max_rows_for(width) rows each (cap > 0: at most cap), min_len over
// len_of(plan row).
template <typename LenOf>
int cut_passes(mv_handle* h, Plan& pl, int start, int end, int width, int cap, LenOf len_of) {
  int rows = max_rows_for(h, width);
  if (cap > 0 && cap < rows) rows = cap;
  if (rows <= 0) return fail(h, MV_ERR_CAPACITY, "mv_config.max_tokens too small for one row of this length");
  for (int first = start; first < end; first += rows) {
    const int n = end - first < rows ? end - first : rows;
    int m = INT32_MAX;
    for (int i = first; i < first + n; ++i) m = std::min(m, (int)len_of(i));
    pl.passes.push_back({first, n, width, m, pl.tokens});
    pl.tokens += (int64_t)n * width;
  }
  return MV_OK;
}

// plan_batch: rows [0, B) of lengths `lens` into pl.  by_length false: the identity order in passes of max_rows_for(S) rows at width S.  by_length true
// (mv_forward_ragged*: a pad-to-longest batch of UNSORTED rows): the rows ordered (stably) by the padded length of their own token count, a run of one padded
// length merged into the next longer one while it holds fewer than min_tokens padded tokens, each group then cut into passes of max_rows_for(its width) rows.
// max_rows > 0 caps the rows of a pass further (the resident sweep's batch).
int plan_batch(mv_handle* h, const int32_t* lens, int B, int S, int min_tokens, bool by_length, int max_rows, Plan& pl) {
  pl.order.clear(), pl.passes.clear(), pl.tokens = 0;
  auto len_of = [&](int i) { return lens[pl.order.empty() ? i : pl.order[i]]; };  // of plan row i
  if (!by_length) return cut_passes(h, pl, 0, B, S, max_rows, len_of);
  auto pad = [&](int r) { return padded_len(lens[r] < 1 ? 1 : lens[r]); };  // of caller row r
  pl.order.resize(B);
  for (int i = 0; i < B; ++i) {
    if (lens[i] > S) return fail(h, MV_ERR_INVALID, "a row is longer than S");
    pl.order[i] = i;
  }
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return pad(a) < pad(b); });
  int start = 0;
  for (int end = 1; end <= B; ++end) {
    const int width = pad(pl.order[end - 1]);
    if (end < B && pad(pl.order[end]) == width) continue;                   // inside a run of one padded length
    if (end < B && (int64_t)(end - start) * width < min_tokens) continue;  // too small a pass: these rows travel with the next longer group
    if (int rc = cut_passes(h, pl, start, end, width < S ? width : S, max_rows, len_of)) return rc;
    start = end;
  }
  return MV_OK;
}

// The form and the anchor count in force when a job is made (MV_F16 has no forms)
void job_form(const mv_handle* h, Job& j) {
  j.G = h->n_anchors;
  j.safe = h->precise && h->form == MV_FORM_SAFE;
  j.guard = h->precise && h->form == MV_FORM_GUARDED;
}

// The one pass loop: the passes [p0, p1) of pl enqueued on workspace set wk without waiting; after a failure it waits for what was enqueued.  Host ids /
// lengths: one upload when they fit wk's buffers, else one per pass at its own width.  Host results: one download each when the rows fit wk's max_batch
// rows (every pass writes at its own rows there), else one per pass.
int run_passes(mv_handle* h, Work& wk, const Plan& pl, size_t p0, size_t p1, const Job& j) {
  const int G = j.G;
  const size_t P = (size_t)h->P;
  const Pass &a = pl.passes[p0], &z = pl.passes[p1 - 1];
  const int rows = z.first + z.rows - a.first;
  const int64_t tokens = z.tok + (int64_t)z.rows * z.width - a.tok;
  const bool one_down = rows <= h->cfg.max_batch, one_up = one_down && tokens <= h->cap_tokens;
  auto upload = [&](int first, int n, int64_t tok, int64_t n_tok) -> int {
    HIPCHK(h, hipMemcpyAsync(wk.d_ids, j.ids + tok, (size_t)n_tok * 4, hipMemcpyHostToDevice, wk.stream));
    HIPCHK(h, hipMemcpyAsync(wk.d_lens, j.lens + first, (size_t)n * 4, hipMemcpyHostToDevice, wk.stream));
    return MV_OK;
  };
  auto download = [&](int first, int n) -> int {  // plan rows [first, first + n) from rows [0, n) of wk's buffers
    const Stage& o = j.out;
    const size_t bg = (size_t)n * G;
    if (o.logits) HIPCHK(h, hipMemcpyAsync(o.logits + (size_t)first * G * 2, wk.logits, bg * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.probs) HIPCHK(h, hipMemcpyAsync(o.probs + (size_t)first * G * 2, wk.probs, bg * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.best) HIPCHK(h, hipMemcpyAsync(o.best + (size_t)first * 2, wk.best, (size_t)n * 8, hipMemcpyDeviceToHost, wk.stream));
    if (o.idx) HIPCHK(h, hipMemcpyAsync(o.idx + first, wk.best_idx, (size_t)n * 4, hipMemcpyDeviceToHost, wk.stream));
    if (o.embed) HIPCHK(h, hipMemcpyAsync(o.embed + (size_t)first * P, wk.u, (size_t)n * P * 4, hipMemcpyDeviceToHost, wk.stream));
    if (o.over) HIPCHK(h, hipMemcpyAsync(o.over + first, wk.seq_over, (size_t)n * 4, hipMemcpyDeviceToHost, wk.stream));
    return MV_OK;
  };
  auto run = [&]() -> int {
    if (j.ids && one_up)
      if (int rc = upload(a.first, rows, a.tok, tokens)) return rc;
    for (size_t i = p0; i < p1; ++i) {
      const Pass& p = pl.passes[i];
      const int32_t* ids = j.ids ? wk.d_ids + (one_up ? p.tok - a.tok : 0) : h->corpus.ids + (size_t)(j.c_row + p.first) * h->corpus.S;
      const int32_t* lens = j.ids ? wk.d_lens + (one_up ? p.first - a.first : 0) : h->corpus.lens + j.c_row + p.first;
      if (j.ids && !one_up)
        if (int rc = upload(p.first, p.rows, p.tok, (int64_t)p.rows * p.width)) return rc;
      const size_t r = one_down ? (size_t)(p.first - a.first) : 0;  // the pass's first row in wk's buffers
      float* u = j.u_dev ? j.u_dev + (size_t)p.first * P : wk.u + r * P;
      PassForm pf;
      pf.safe = j.safe; pf.monitor = j.monitor;
      if (j.guard) {
        pf.seq_over = j.ids ? wk.seq_over + r : h->corpus.over + j.c_row + p.first;
        HIPCHK(h, hipMemsetAsync(pf.seq_over, 0, (size_t)p.rows * 4, wk.stream));
      }
      if (int rc = encode_dev(h, wk, ids, lens, p.min_len, p.rows, p.width, j.n_layers, u, pf, j.full, j.ids ? p.width : h->corpus.S)) return rc;
      if (!j.ids) {
        const size_t c = (size_t)(j.c_row + p.first);
        if (int rc = match_dev(h, wk, u, p.rows, G, nullptr, nullptr, j.keep_psame ? h->corpus.psame + c * G : nullptr, j.topk ? j.topk : 1, h->corpus.best + c * 2, h->corpus.idx + c,
                               j.topk ? h->corpus.topk_p + c * j.topk : nullptr, j.topk ? h->corpus.topk_idx + c * j.topk : nullptr)) return rc;
      } else if (j.match) {  // only the outputs the caller asked for leave the kernel (the best anchor always does)
        if (int rc = match_dev(h, wk, u, p.rows, G, j.out.logits ? wk.logits + r * G * 2 : nullptr, j.out.probs ? wk.probs + r * G * 2 : nullptr, nullptr, 1,
                               wk.best + r * 2, wk.best_idx + r)) return rc;
      }
      if (!one_down)
        if (int rc = download(p.first, p.rows)) return rc;
    }
    return one_down ? download(a.first, rows) : MV_OK;
  };
  const int rc = run();
  if (rc != MV_OK) hipStreamSynchronize(wk.stream);
  return rc;
}

// The one row scatter: row i of src to row map[i] of dst (an empty map: to row i), n rows — the results both hold.
void scatter_rows(const Stage& src, const Stage& dst, const std::vector<int>& map, size_t n, size_t G, size_t P) {
  const size_t g2 = G * 2;
  for (size_t i = 0; i < n; ++i) {
    const size_t o = map.empty() ? i : (size_t)map[i];
    if (src.logits && dst.logits) std::memcpy(dst.logits + o * g2, src.logits + i * g2, g2 * 4);
    if (src.probs && dst.probs) std::memcpy(dst.probs + o * g2, src.probs + i * g2, g2 * 4);
    if (src.best && dst.best) { dst.best[o * 2] = src.best[i * 2]; dst.best[o * 2 + 1] = src.best[i * 2 + 1]; }
    if (src.idx && dst.idx) dst.idx[o] = src.idx[i];
    if (src.embed && dst.embed) std::memcpy(dst.embed + o * P, src.embed + i * P, P * 4);
  }
}

// ---- the guarded form -------------------------------------------------------------------------------------------------------------------------------------
// The rule, per sequence: rescored in the safe form when more than kGuardShare of the (head, layer) items the monitor looked at for it are over MV_SINK_COLLISION
// (attention.h) — the 2 % rule of binding.Engine._check_saturation applied to one sequence.  The monitor looks at every head of every layer whose attention runs
// through attention_v2_kernel (the pruned last layer's single-query attention feeds none), for sequences of at least 16 tokens.
constexpr double kGuardShare = 0.02;
bool guard_flagged(const mv_handle* h, uint32_t over, int len) {
  const int layers = h->cfg.layers - ((h->cls_prune && h->cfg.layers > 0) ? 1 : 0);
  const int items = len >= 16 ? MV_HEADS * layers : 0;
  return (double)over > kGuardShare * (double)items;
}

// After the default-form passes of a guarded job (j.out.over holds the counts, the stream is idle): a second plan over the flagged rows — each at the width of
// the pass it first ran in, the flagged rows of every pass of one width sharing passes — run in the safe form with the monitor detached, against the job's own
// anchor count; those rows' results in j.out (and in the bank, j.u_dev: one copy per row) are overwritten.  Records the form of each of the B rows in the
// caller's order (mv_last_row_forms).
int rescore_rows(mv_handle* h, Work& wk, const Plan& pl, const Job& j, int B) {
  h->last_forms.assign((size_t)B, (uint8_t)(j.safe ? MV_FORM_SAFE : MV_FORM_DEFAULT));
  if (!j.guard) return MV_OK;
  h->guard_seqs += B;
  Plan& p2 = h->plan2;
  HostStage& v = h->stage2;
  p2.order.clear(), p2.passes.clear(), p2.tokens = 0;
  v.ids.clear(), v.lens.clear();
  std::vector<int> widths;
  int64_t n_routed = 0;
  for (const Pass& p : pl.passes)
    if (std::find(widths.begin(), widths.end(), p.width) == widths.end()) widths.push_back(p.width);
  for (const int w : widths) {
    const int start = (int)p2.order.size();
    for (const Pass& p : pl.passes) {
      if (p.width != w) continue;
      for (int i = 0; i < p.rows; ++i) {
        const int r = p.first + i;
        const bool forced = j.routed && j.routed[r];  // (its count was never written)
        if (!forced && !guard_flagged(h, j.out.over[r], j.lens[r])) continue;
        n_routed += forced;
        p2.order.push_back(r);
        v.lens.push_back(j.lens[r]);
        const int32_t* src = j.ids + p.tok + (int64_t)i * w;
        v.ids.insert(v.ids.end(), src, src + w);
      }
    }
    if (int rc = cut_passes(h, p2, start, (int)p2.order.size(), w, 0, [&](int i) { return v.lens[(size_t)i]; })) return rc;
  }
  const size_t n2 = p2.order.size(), P = (size_t)h->P;
  if (!n2) return MV_OK;
  Job r;
  r.match = j.match; r.G = j.G; r.safe = true; r.monitor = false;
  r.out = v.view(n2, (size_t)p2.tokens, (size_t)j.G, P, wanted(j.out, j.out.embed || j.u_dev));  // (the ids and the lengths are in it already)
  r.ids = r.out.ids; r.lens = r.out.lens;
  if (int rc = run_passes(h, wk, p2, 0, p2.passes.size(), r)) return rc;
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  scatter_rows(r.out, j.out, p2.order, n2, (size_t)j.G, P);
  for (size_t i = 0; i < n2; ++i) {
    const size_t o = (size_t)p2.order[i];
    if (j.u_dev) HIPCHK(h, hipMemcpyAsync(j.u_dev + o * P, r.out.embed + i * P, P * 4, hipMemcpyHostToDevice, wk.stream));
    h->last_forms[pl.order.empty() ? o : (size_t)pl.order[o]] = MV_FORM_SAFE;
  }
  if (j.u_dev) HIPCHK(h, hipStreamSynchronize(wk.stream));
  h->guard_rescored += (int64_t)n2 - n_routed;
  h->routed_seqs += n_routed;
  return MV_OK;
}

// ---- the sink-token list (mv_set_sink_tokens; route.h) ----------------------------------------------------------------------------------------------------------
// A host batch of a guarded job: the rows of [B][S] the list routes (h->route_flags, caller's row order); returns how many.  0 without a list.
int scan_routed(mv_handle* h, const Job& j, const int32_t* ids, const int32_t* lens, int B, int S) {
  if (!j.guard || j.full || h->sink_tokens.empty()) return 0;
  h->route_flags.resize((size_t)B);
  return route_scan(ids, lens, B, S, h->sink_bitmap.data(), h->cfg.vocab_size, h->route_flags.data());
}

// A planned batch with routed rows (flags: caller's row order): every pass of pl keeps its rows and its width, with its unrouted rows first — pl.order is made
// explicit for that — `routed` marks the others in plan order, and p1 gets one pass per pass of pl that has unrouted rows: those rows alone, min_len over them
// (the ids of a pass are staged in plan order, so they are the head of the pass's ids: same Pass::tok).
void split_plan(Plan& pl, int B, const int32_t* lens, const uint8_t* flags, std::vector<uint8_t>& routed, Plan& p1) {
  if (pl.order.empty()) {
    pl.order.resize((size_t)B);
    for (int i = 0; i < B; ++i) pl.order[(size_t)i] = i;
  }
  routed.assign((size_t)B, 0);
  p1.order.clear(), p1.passes.clear(), p1.tokens = pl.tokens;
  for (const Pass& p : pl.passes) {
    const auto b = pl.order.begin() + p.first, e = b + p.rows;
    const auto mid = std::stable_partition(b, e, [&](int r) { return !flags[r]; });
    const int nu = (int)(mid - b);
    for (int i = nu; i < p.rows; ++i) routed[(size_t)(p.first + i)] = 1;
    if (!nu) continue;
    int m = INT32_MAX;
    for (auto it = b; it != mid; ++it) m = std::min(m, lens[*it]);
    p1.passes.push_back({p.first, nu, p.width, m, p.tok});
  }
}

// ---- the one host batch flow --------------------------------------------------------------------------------------------------------------------------------------
// The rows of a batch gathered into plan order: each pass's ids at its own width (ids [B][S]).
void gather(const Plan& pl, const int32_t* ids, const int32_t* lens, int S, int32_t* ids_out, int32_t* lens_out) {
  for (const Pass& p : pl.passes)
    for (int i = 0; i < p.rows; ++i) {
      const size_t r = (size_t)pl.order[p.first + i];
      std::memcpy(ids_out + p.tok + (int64_t)i * p.width, ids + r * S, (size_t)p.width * 4);
      lens_out[p.first + i] = lens[r];
    }
}

// Make and enqueue: rows [0, B) of ids [B][S] planned into pl (plan_batch), the rows the sink-token list routes split off (scan_routed, split_plan: `routed`,
// which j then points into), the batch gathered in plan order into a view of the staging — hs, or wk's pinned one — that holds the results `want` names, and the
// passes of the unrouted rows enqueued on wk.  Does not wait.  j comes in made (match, form, anchor count) and leaves with the staging as its ids, lens and out.
// A batch in its own order with no routed row is not staged: its ids are read in place and j.out stays the caller's arrays (the plan's order is empty).
int enqueue_batch(mv_handle* h, Work& wk, Plan& pl, std::vector<uint8_t>& routed, HostStage* hs, const int32_t* ids, const int32_t* lens, int B, int S,
                  int min_tokens, bool by_length, Want want, Job& j) {
  if (int rc = plan_batch(h, lens, B, S, min_tokens, by_length, 0, pl)) return rc;
  const Plan* p1 = &pl;  // the passes of the first run: without the routed rows
  routed.clear();
  j.routed = nullptr;
  if (scan_routed(h, j, ids, lens, B, S)) {
    split_plan(pl, B, lens, h->route_flags.data(), routed, h->plan1);
    j.routed = routed.data();
    p1 = &h->plan1;
  }
  const bool in_place = pl.order.empty();
  if (in_place) want = Want();  // (only the monitor counts go through the staging)
  want.over = j.guard;
  const Stage st = hs ? hs->view((size_t)B, in_place ? 0 : (size_t)pl.tokens, (size_t)j.G, (size_t)h->P, want) : only(wk.pin, want);
  if (in_place) {
    j.ids = ids; j.lens = lens; j.out.over = st.over;
  } else {
    gather(pl, ids, lens, S, st.ids, st.lens);
    j.ids = st.ids; j.lens = st.lens; j.out = st; j.u_dev = nullptr;
  }
  return p1->passes.empty() ? MV_OK : run_passes(h, wk, *p1, 0, p1->passes.size(), j);
}

// Collect: wait for wk, rescore the flagged and the routed rows of a guarded job (rescore_rows), and bring a staged batch's results to the caller's rows (dst).
int collect_batch(mv_handle* h, Work& wk, const Plan& pl, const Job& j, int B, const Stage& dst) {
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  if (!j.full)  // (mv_debug_encode: the taps show the passes as they ran)
    if (int rc = rescore_rows(h, wk, pl, j, B)) return rc;
  if (!pl.order.empty()) scatter_rows(j.out, dst, pl.order, (size_t)B, (size_t)j.G, (size_t)h->P);
  return MV_OK;
}

// mv_forward / mv_encode / mv_anchor_append / mv_debug_encode: the rows in their own order on workspace set 0, both halves back to back.  mv_anchor_append with
// routed rows (the batch was staged): the bank's rows in the caller's order, in one copy.
int run_in_order(mv_handle* h, const int32_t* lens, int B, int S, const Job& j) {
  Work& wk = h->work[0];
  const size_t P = (size_t)h->P;
  Job s = j;
  if (int rc = enqueue_batch(h, wk, h->plan, h->routed, &h->stage, j.ids, lens, B, S, 0, false, wanted(j.out, j.out.embed || j.u_dev), s)) return rc;
  if (int rc = collect_batch(h, wk, h->plan, s, B, j.out)) return rc;
  if (j.u_dev && !h->plan.order.empty()) {
    Want e;
    e.embed = true;
    const Stage bank = h->stage2.view((size_t)B, 0, 0, P, e);  // (rescore_rows is done with it)
    scatter_rows(s.out, bank, h->plan.order, (size_t)B, 0, P);
    HIPCHK(h, hipMemcpyAsync(j.u_dev, bank.embed, (size_t)B * P * 4, hipMemcpyHostToDevice, wk.stream));
    HIPCHK(h, hipStreamSynchronize(wk.stream));
  }
  return MV_OK;
}

}  // namespace
