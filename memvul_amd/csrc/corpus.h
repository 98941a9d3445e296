// Part of engine.hip: the resident corpus (Corpus, engine.hip) — its reset (release_corpus), its shared preconditions (corpus_ready, kept_rows_ready), the
// P(same) sizing (ensure_psame), the indexed pass and the guarded form's rescoring over it, the routing flags, and the mv_corpus_* entries.

namespace {

// The one indexed pass over the resident corpus: rows idx[0, n) gathered into wk's pass buffer at width w, encoded in the form pf (counts: with the per-row
// monitor counts kept), matched, and scattered back to their corpus slots — keep: their P(same) rows too, counts: the counts to Corpus::over; on a keeping corpus
// (mv_corpus_keep) their embeddings and top-k lists as well: a flagged or routed row holds the safe form's, like its best anchor.  Asynchronous on wk:
// idx stays alive until that stream has been waited for; after a failure it waits for what it enqueued.
int run_corpus_rows(mv_handle* h, Work& wk, const int32_t* idx, int n, int w, int min_len, PassForm pf, bool keep, bool counts) {
  const Corpus& c = h->corpus;
  const int G = h->n_anchors;
  auto run = [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(wk.d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, wk.stream));
    const int64_t nt = (int64_t)n * w;
    hipLaunchKernelGGL(corpus_gather_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, wk.stream, (const int32_t*)c.ids, (const int32_t*)c.lens,
                       c.S, (const int32_t*)wk.d_idx, n, w, wk.d_ids, wk.d_lens);
    if (int rc = launch_check(h, "corpus_gather")) return rc;
    if (counts) {
      pf.seq_over = wk.seq_over;
      HIPCHK(h, hipMemsetAsync(pf.seq_over, 0, (size_t)n * 4, wk.stream));
    }
    if (int rc = encode_dev(h, wk, wk.d_ids, wk.d_lens, min_len, n, w, -1, wk.u, pf, false, w)) return rc;
    const int k = c.k;  // mv_corpus_keep: the rows' top-k lists (and their embeddings, wk.u) go back to their corpus slots too
    if (int rc = match_dev(h, wk, wk.u, n, G, nullptr, nullptr, keep ? wk.psame : nullptr, k ? k : 1, wk.best, wk.best_idx, k ? wk.topk_p : nullptr,
                           k ? wk.topk_idx : nullptr)) return rc;
    const int64_t ns = (int64_t)n * (keep ? G : 1);
    hipLaunchKernelGGL(corpus_scatter_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, wk.stream, (const float*)wk.best, (const int32_t*)wk.best_idx,
                       keep ? (const float*)wk.psame : (const float*)nullptr, (const int32_t*)wk.d_idx, n, G, c.best, c.idx, c.psame,
                       counts ? (const uint32_t*)wk.seq_over : (const uint32_t*)nullptr, counts ? c.over : (uint32_t*)nullptr);
    if (int rc = launch_check(h, "corpus_scatter")) return rc;
    if (!c.embed && !k) return MV_OK;
    const int64_t nk = (int64_t)n * ((c.embed ? h->P / 4 : 0) + 2 * ((k & 3) ? k : k / 4));  // one thread per 16 bytes (corpus_scatter_keep_kernel)
    hipLaunchKernelGGL(corpus_scatter_keep_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, wk.stream, c.embed ? (const float*)wk.u : (const float*)nullptr,
                       (const uint32_t*)wk.topk_p, (const uint32_t*)wk.topk_idx, (const int32_t*)wk.d_idx, n, h->P, k, c.embed, (uint32_t*)c.topk_p,
                       (uint32_t*)c.topk_idx);
    return launch_check(h, "corpus_scatter_keep");
  };
  const int rc = run();
  if (rc != MV_OK) hipStreamSynchronize(wk.stream);
  return rc;
}

// The resident corpus: every row a guarded sweep ran since the last rescoring (Corpus::pend) whose count (Corpus::over) flags it, and every row it left out as routed —
// grouped by the s_eff width of the run (and whether it kept P(same)), each group cut into full passes and run through run_corpus_rows in the safe form with the
// monitor detached.  On workspace set 0, after every batch of the sweep has finished; waits once, at the end.
int rescore_corpus(mv_handle* h) {
  Corpus& c = h->corpus;
  if (!c.pending) return MV_OK;
  if (int rc = sync_all(h)) return rc;
  c.pending = false;
  c.idx_live.clear();
  Work& wk = h->work[0];
  std::vector<uint32_t> over((size_t)c.n);
  HIPCHK(h, hipMemcpyAsync(over.data(), c.over, (size_t)c.n * 4, hipMemcpyDeviceToHost, wk.stream));
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  std::map<int, std::vector<int32_t>> groups;  // 2 width + keep -> corpus rows (alive until the last upload from them has been waited for)
  for (int64_t r = 0; r < c.n; ++r) {
    const int w = c.pend[(size_t)r].w;
    if (!w) continue;
    c.pend[(size_t)r].w = 0;
    const int forced = c.pend[(size_t)r].force;  // routed by the sink-token list of its sweep: it has run in no pass yet
    if (forced || guard_flagged(h, over[(size_t)r], c.lens_host[(size_t)r])) groups[2 * w + c.pend[(size_t)r].keep].push_back((int32_t)r);
  }
  PassForm pf;
  pf.safe = true; pf.monitor = false;
  for (auto& kv : groups) {
    const int w = kv.first >> 1;
    const bool keep = (kv.first & 1) && c.psame && c.G == h->n_anchors;
    const std::vector<int32_t>& idx = kv.second;
    Plan g;  // the group's rows in passes
    if (int rc = cut_passes(h, g, 0, (int)idx.size(), w, 0, [&](int i) { return c.lens_host[(size_t)idx[(size_t)i]]; })) return rc;
    for (const Pass& p : g.passes) {
      if (int rc = run_corpus_rows(h, wk, idx.data() + p.first, p.rows, w, p.min_len, pf, keep, false)) return rc;
      for (int i = p.first; i < p.first + p.rows; ++i) {
        c.forms[(size_t)idx[(size_t)i]] = MV_FORM_SAFE;
        (c.pend[(size_t)idx[(size_t)i]].force ? h->routed_seqs : h->guard_rescored) += 1;
      }
    }
  }
  HIPCHK(h, hipStreamSynchronize(wk.stream));
  return MV_OK;
}

// The resident corpus: h->corpus.route = the flag of every row under the current list, recomputed when an upload or a list change made it stale — one kernel over
// the whole corpus, one copy back, one wait (workspace set 0's stream; nothing on the device reads what it writes).  An empty list flags nothing, without a launch.
int ensure_route_flags(mv_handle* h) {
  Corpus& c = h->corpus;
  if (!c.route_stale) return MV_OK;
  c.route.assign((size_t)c.n, 0);
  if (!h->sink_tokens.empty() && c.n > 0) {
    const hipStream_t s0 = h->work[0].stream;
    if (!h->route_bm_dev)
      if (int rc = dev_alloc(h, s0, &h->route_bm_dev, (int64_t)h->sink_bitmap.size(), false)) return rc;
    if (!c.route_dev)
      if (int rc = dev_alloc(h, s0, &c.route_dev, c.n, false)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->route_bm_dev, h->sink_bitmap.data(), h->sink_bitmap.size() * 4, hipMemcpyHostToDevice, s0));
    hipLaunchKernelGGL(route_flags_kernel, dim3((unsigned)((c.n + 3) / 4)), dim3(256), 0, s0, (const int32_t*)c.ids, (const int32_t*)c.lens, c.n, c.S,
                       (const uint32_t*)h->route_bm_dev, h->cfg.vocab_size, c.route_dev);
    if (int rc = launch_check(h, "route_flags")) return rc;
    HIPCHK(h, hipMemcpyAsync(c.route.data(), c.route_dev, (size_t)c.n, hipMemcpyDeviceToHost, s0));
    HIPCHK(h, hipStreamSynchronize(s0));
  }
  c.route_stale = false;
  return MV_OK;
}

// One batch of a guarded sweep that has routed rows (pass p of the sweep's plan, whose row 0 is corpus row j.c_row): its unrouted rows through run_corpus_rows
// at the sweep's width, in the default form with the per-row monitor counts kept.  Asynchronous, like the in-place batches next to it: the index list lives in
// Corpus::idx_live until rescore_corpus has waited for the sweep.
int run_split_batch(mv_handle* h, Work& wk, const Pass& p, const Job& j) {
  std::vector<int32_t> idx;
  int m = INT32_MAX;
  for (int i = 0; i < p.rows; ++i) {
    const int64_t r = j.c_row + p.first + i;
    if (h->corpus.route[(size_t)r]) continue;
    idx.push_back((int32_t)r);
    m = std::min(m, h->corpus.lens_host[(size_t)r]);
  }
  if (idx.empty()) return MV_OK;  // every row routed: nothing runs in the default form
  h->corpus.idx_live.push_back(std::move(idx));
  const std::vector<int32_t>& ix = h->corpus.idx_live.back();
  return run_corpus_rows(h, wk, ix.data(), (int)ix.size(), p.width, m, PassForm(), j.keep_psame, true);
}

// What every corpus entry asks first, before its own arguments: a handle — ANY: nothing more; FINAL: finalised weights; IDLE: as check_ready, the sweeps on the
// other workspace sets waited for — and an uploaded corpus.
enum CorpusReady { CORPUS_ANY, CORPUS_FINAL, CORPUS_IDLE };
int corpus_ready(mv_handle* h, CorpusReady how) {
  if (!h) return MV_ERR_INVALID;
  if (how != CORPUS_ANY)
    if (int rc = how == CORPUS_IDLE ? check_ready(h) : check_final(h)) return rc;
  if (!h->corpus.ids) return fail(h, MV_ERR_STATE, "no resident corpus (mv_corpus_upload)");
  return MV_OK;
}

// Every device array the corpus owns, freed (mv_corpus_upload then starts from Corpus{}).  The stream that wrote them has been waited for.
void release_corpus(mv_handle* h) {
  const Corpus& c = h->corpus;
  for (void* p : std::initializer_list<void*>{c.ids, c.lens, c.best, c.idx, c.psame, c.over, c.embed, c.topk_p, c.topk_idx, c.route_dev}) dev_free(h, p);
}

// P(same) [n][G] sized for this corpus and a bank of G anchors: allocated (zeroed, on set 0's stream) at the first keeping run and again when either changed.
// sync_first: batches of a sweep may still write the old array — wait for every set before it is freed.
int ensure_psame(mv_handle* h, int G, bool sync_first) {
  Corpus& c = h->corpus;
  if (c.psame_rows == c.n && c.G == G) return MV_OK;
  if (sync_first)
    if (int rc = sync_all(h)) return rc;
  dev_free(h, c.psame);
  c.psame = nullptr;
  if (int rc = dev_alloc(h, h->work[0].stream, &c.psame, c.n * G)) return rc;
  c.psame_rows = c.n;
  c.G = G;
  return MV_OK;
}

// mv_corpus_keep in force at a run against G anchors: k checked against the bank, and the arrays allocated at the first such run (like Corpus::psame).  The zeroing
// runs on set 0's stream and the batches may start on the other one: it is waited for here, once.
int keep_prepare(mv_handle* h, int G) {
  Corpus& c = h->corpus;
  const int k = c.k;
  if (!c.keep_embed && !k) return MV_OK;
  if (k > G) return fail(h, MV_ERR_INVALID, "mv_corpus_run: the kept top-k (mv_corpus_keep) exceeds the number of anchors");
  if ((int64_t)(G <= 128 ? 1 : (G + 255) / 256) * k > 1024) return fail(h, MV_ERR_INVALID, "top-k: anchors / 256 * k must not exceed 1024");
  const hipStream_t s0 = h->work[0].stream;
  bool fresh = false;
  auto alloc = [&](auto** p, int64_t count, const char* what) -> int {
    if (*p) return MV_OK;
    fresh = true;
    const int rc = dev_alloc(h, s0, p, count);
    if (rc != MV_ERR_NOMEM) return rc;
    return fail(h, MV_ERR_NOMEM, "mv_corpus_run: cannot allocate " + std::to_string((long long)count * 4) + " bytes for the kept " + what + " (mv_corpus_keep): " + h->err);
  };
  if (c.keep_embed)
    if (int rc = alloc(&c.embed, c.n * h->P, "embeddings")) return rc;
  if (k) {
    if (int rc = alloc(&c.topk_p, c.n * k, "top-k probabilities")) return rc;
    if (int rc = alloc(&c.topk_idx, c.n * k, "top-k indices")) return rc;
  }
  if (fresh) HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
}

// The checks the three readers of the kept arrays share, after corpus_ready: the corpus keeps it, a range inside it, every row of it covered by a keeping run —
// then what mv_corpus_results collects first (the sweeps in flight, the guarded form's rescoring).
int kept_rows_ready(mv_handle* h, const char* who, int64_t first, int64_t count, bool kept) {
  if (!kept) return fail(h, MV_ERR_STATE, std::string(who) + ": the corpus does not keep that (mv_corpus_keep)");
  if (first < 0 || count <= 0 || first + count > h->corpus.n || count > INT32_MAX) return fail(h, MV_ERR_INVALID, std::string(who) + ": bad range");
  for (int64_t r = first; r < first + count; ++r)
    if (!h->corpus.has[(size_t)r]) return fail(h, MV_ERR_STATE, std::string(who) + ": row " + std::to_string((long long)r) + " has not been swept by a keeping run");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  return rescore_corpus(h);
}

}  // namespace

extern "C" {

// ---- resident corpus ---------------------------------------------------------------------------
int mv_corpus_upload(mv_handle* h, const int32_t* ids, const int32_t* lens, int64_t n, int S) try {
  if (int rc = check_ready(h)) return rc;
  if (!ids || !lens || n <= 0 || S <= 0 || S > h->cfg.max_pos) return fail(h, MV_ERR_INVALID, "mv_corpus_upload: bad argument");
  if (int rc = check_ids(h, ids, n * S, "mv_corpus_upload")) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const hipStream_t s0 = h->work[0].stream;
  HIPCHK(h, hipStreamSynchronize(s0));
  release_corpus(h);
  h->corpus = Corpus{};
  Corpus& c = h->corpus;
  if (int rc = dev_alloc(h, s0, &c.ids, n * S, false)) return rc;
  if (int rc = dev_alloc(h, s0, &c.lens, n, false)) return rc;
  if (int rc = dev_alloc(h, s0, &c.best, n * 2)) return rc;
  if (int rc = dev_alloc(h, s0, &c.idx, n)) return rc;
  if (int rc = dev_alloc(h, s0, &c.over, n)) return rc;
  c.pend.assign((size_t)n, Corpus::Pending{});  // the per-row vectors, sized here (has: mv_corpus_keep; route: ensure_route_flags)
  c.forms.assign((size_t)n, MV_FORM_DEFAULT);
  HIPCHK(h, hipMemcpyAsync(c.ids, ids, (size_t)n * S * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipMemcpyAsync(c.lens, lens, (size_t)n * 4, hipMemcpyHostToDevice, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  c.lens_host.assign(lens, lens + n);
  c.n = n;
  c.S = S;
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_run(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs) try {
  return mv_corpus_run_len(h, first, count, batch, keep_probs, 0);
} catch (...) { return on_exception(h); }

int mv_corpus_run_len(mv_handle* h, int64_t first, int64_t count, int batch, int keep_probs, int s_eff) try {
  if (int rc = corpus_ready(h, CORPUS_FINAL)) return rc;
  Corpus& c = h->corpus;
  if (first < 0 || count <= 0 || first + count > c.n || count > INT32_MAX || batch <= 0) return fail(h, MV_ERR_INVALID, "mv_corpus_run: bad range");
  if (h->n_anchors <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty");
  HIPCHK(h, hipSetDevice(h->device));
  if (s_eff < 0 || s_eff > c.S) return fail(h, MV_ERR_INVALID, "mv_corpus_run_len: s_eff must be in [0, S of the resident corpus]");
  // tokens per row actually processed (rows longer than this must not be in the range); a batch larger than one pass holds is walked in passes (as
  // mv_forward / mv_encode do): a row's result does not depend on the batch it travels in (bit-identical, tests/test_gpu_parity.py::test_full_batch_properties)
  const int S_use = s_eff > 0 ? s_eff : c.S;
  Plan& pl = h->plan;
  if (int rc = plan_batch(h, c.lens_host.data() + first, (int)count, S_use, 0, false, batch, pl)) return rc;
  const int G = h->n_anchors;
  if (keep_probs)
    if (int rc = ensure_psame(h, G, true)) return rc;
  if (int rc = keep_prepare(h, G)) return rc;
  c.ran = true;
  // consecutive batches (also across calls) alternate between the two workspace sets / streams: two batches are in
  // flight at once; their results go to disjoint slices of the resident arrays
  Job j;
  j.c_row = first; j.keep_psame = keep_probs != 0;
  job_form(h, j);
  if (c.embed) j.u_dev = c.embed + (size_t)first * h->P;  // a keeping sweep: the encoder writes the rows' slots, the matcher reads them there
  j.topk = c.k;
  if (!c.has.empty()) std::fill(c.has.begin() + first, c.has.begin() + first + count, (uint8_t)1);
  // ... with a sink-token list: the rows it routes run in no batch here, they are marked pending and forced (rescore_corpus encodes them in the safe form)
  const bool route = j.guard && !h->sink_tokens.empty();
  if (route)
    if (int rc = ensure_route_flags(h)) return rc;
  // the guarded form: the sweep stays asynchronous and only records the per-row counts (Corpus::over) and what it ran (Corpus::pend): rescore_corpus, from mv_corpus_results
  for (int64_t r = first; r < first + count; ++r) {
    c.pend[(size_t)r].force = (uint8_t)(route && c.route[(size_t)r]);
    c.pend[(size_t)r].w = (int16_t)(j.guard ? S_use : 0);
    c.pend[(size_t)r].keep = (uint8_t)(keep_probs != 0);
    c.forms[(size_t)r] = (uint8_t)(j.safe ? MV_FORM_SAFE : MV_FORM_DEFAULT);
  }
  if (j.guard) { c.pending = true; h->guard_seqs += count; }
  for (size_t i = 0; i < pl.passes.size(); ++i) {
    Work& wk = h->work[h->rr];
    wk.sweep = true;
    if (h->n_streams == 2) h->rr ^= 1;
    const Pass& p = pl.passes[i];
    const uint8_t* f = route ? c.route.data() + first + p.first : nullptr;
    if (f && std::find(f, f + p.rows, (uint8_t)1) != f + p.rows) {  // (a batch with no routed row takes the in-place path)
      if (int rc = run_split_batch(h, wk, p, j)) return rc;
      continue;
    }
    if (int rc = run_passes(h, wk, pl, i, i + 1, j)) return rc;
  }
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_results(mv_handle* h, int64_t first, int64_t count, float* best, int32_t* best_idx, float* p_same) try {
  if (int rc = corpus_ready(h, CORPUS_ANY)) return rc;
  const Corpus& c = h->corpus;
  if (first < 0 || count <= 0 || first + count > c.n) return fail(h, MV_ERR_INVALID, "mv_corpus_results: bad range");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_all(h)) return rc;
  if (int rc = rescore_corpus(h)) return rc;
  const hipStream_t s0 = h->work[0].stream;
  if (best) HIPCHK(h, hipMemcpyAsync(best, c.best + (size_t)first * 2, (size_t)count * 8, hipMemcpyDeviceToHost, s0));
  if (best_idx) HIPCHK(h, hipMemcpyAsync(best_idx, c.idx + first, (size_t)count * 4, hipMemcpyDeviceToHost, s0));
  if (p_same) {
    if (!c.psame) return fail(h, MV_ERR_STATE, "P(same) was not kept (mv_corpus_run keep_probs=0)");
    HIPCHK(h, hipMemcpyAsync(p_same, c.psame + (size_t)first * c.G, (size_t)count * c.G * 4, hipMemcpyDeviceToHost, s0));
  }
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_keep(mv_handle* h, int keep_embed, int topk) try {
  if (int rc = corpus_ready(h, CORPUS_IDLE)) return rc;
  if ((keep_embed != 0 && keep_embed != 1) || topk < 0 || topk > MK_KMAX) return fail(h, MV_ERR_INVALID, "mv_corpus_keep: keep_embed must be 0 or 1, topk in [0, 64]");
  if (h->corpus.ran) return fail(h, MV_ERR_STATE, "mv_corpus_keep: the corpus has been swept already (call it after mv_corpus_upload, before the first mv_corpus_run)");
  h->corpus.keep_embed = keep_embed;
  h->corpus.k = topk;
  if (keep_embed || topk) h->corpus.has.assign((size_t)h->corpus.n, 0); else h->corpus.has.clear();
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_rematch(mv_handle* h, int64_t first, int64_t count, int g_first, int keep_probs) try {
  if (int rc = corpus_ready(h, CORPUS_IDLE)) return rc;
  Corpus& c = h->corpus;
  if (!c.embed) return fail(h, MV_ERR_STATE, "mv_corpus_rematch: no embeddings kept (mv_corpus_keep before the sweep)");
  const int G = h->n_anchors, k = c.k;
  if (G <= 0) return fail(h, MV_ERR_STATE, "anchor bank is empty");
  if (g_first < 0 || g_first > G) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: g_first must be in [0, number of anchors]");
  if (keep_probs != 0 && keep_probs != 1) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: keep_probs must be 0 or 1");
  if (keep_probs && g_first > 0) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: keep_probs needs g_first == 0 (the pitch of the P(same) rows changes with the bank)");
  if (k > G) return fail(h, MV_ERR_INVALID, "mv_corpus_rematch: the kept top-k exceeds the number of anchors");
  if (int rc = kept_rows_ready(h, "mv_corpus_rematch", first, count, true)) return rc;
  if (g_first == G) return MV_OK;  // nothing was appended
  Work& wk = h->work[0];
  const size_t P = (size_t)h->P;
  if (keep_probs)
    if (int rc = ensure_psame(h, G, false)) return rc;
  auto run = [&]() -> int {
    for (int64_t r = first; r < first + count; r += h->cfg.max_batch) {
      const int nb = (int)std::min<int64_t>(h->cfg.max_batch, first + count - r);
      const float* u = c.embed + (size_t)r * P;  // read in place
      if (g_first == 0) {  // full: the stored results rewritten
        if (int rc = match_dev(h, wk, u, nb, G, nullptr, nullptr, keep_probs ? c.psame + (size_t)r * G : nullptr, k ? k : 1, c.best + r * 2, c.idx + r,
                               k ? c.topk_p + r * k : nullptr, k ? c.topk_idx + r * k : nullptr)) return rc;
        continue;
      }
      // appended: the new anchors alone into the workspace, then folded into the stored results
      const int ks = k ? std::min(k, G - g_first) : 0;
      if (int rc = match_dev(h, wk, u, nb, G - g_first, nullptr, nullptr, nullptr, ks ? ks : 1, wk.best, wk.best_idx, ks ? wk.topk_p : nullptr, ks ? wk.topk_idx : nullptr,
                             g_first)) return rc;
      RematchMergeArgs a{nb, k, ks, g_first, h->cfg.same_idx, wk.best, wk.best_idx, wk.topk_p, wk.topk_idx, c.best + r * 2, c.idx + r,
                         k ? c.topk_p + r * k : nullptr, k ? c.topk_idx + r * k : nullptr};
      ProfScope ps(h, wk.stream, KC_TOPK);
      hipLaunchKernelGGL(rematch_merge_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, wk.stream, a);
      if (int rc = launch_check(h, "rematch_merge")) return rc;
    }
    return MV_OK;
  };
  const int rc = run();
  const hipError_t e = hipStreamSynchronize(wk.stream);
  if (rc != MV_OK) return rc;
  HIPCHK(h, e);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_embeddings(mv_handle* h, int64_t first, int64_t count, float* embed) try {
  if (int rc = corpus_ready(h, CORPUS_IDLE)) return rc;
  if (int rc = kept_rows_ready(h, "mv_corpus_embeddings", first, count, h->corpus.keep_embed != 0)) return rc;
  if (!embed) return fail(h, MV_ERR_INVALID, "mv_corpus_embeddings: bad argument");
  const hipStream_t s0 = h->work[0].stream;
  HIPCHK(h, hipMemcpyAsync(embed, h->corpus.embed + (size_t)first * h->P, (size_t)count * h->P * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_topk(mv_handle* h, int64_t first, int64_t count, float* topk_p, int32_t* topk_idx) try {
  if (int rc = corpus_ready(h, CORPUS_IDLE)) return rc;
  if (int rc = kept_rows_ready(h, "mv_corpus_topk", first, count, h->corpus.k > 0)) return rc;
  if (!topk_p || !topk_idx) return fail(h, MV_ERR_INVALID, "mv_corpus_topk: bad argument");
  const hipStream_t s0 = h->work[0].stream;
  const size_t k = (size_t)h->corpus.k;
  HIPCHK(h, hipMemcpyAsync(topk_p, h->corpus.topk_p + (size_t)first * k, (size_t)count * k * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipMemcpyAsync(topk_idx, h->corpus.topk_idx + (size_t)first * k, (size_t)count * k * 4, hipMemcpyDeviceToHost, s0));
  HIPCHK(h, hipStreamSynchronize(s0));
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_route_flags(mv_handle* h, int64_t first, int64_t count, uint8_t* flags) try {
  if (!h || !flags) return fail(h, MV_ERR_INVALID, "mv_corpus_route_flags: bad argument");
  if (int rc = corpus_ready(h, CORPUS_ANY)) return rc;
  if (first < 0 || count <= 0 || first + count > h->corpus.n) return fail(h, MV_ERR_INVALID, "mv_corpus_route_flags: bad range");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = ensure_route_flags(h)) return rc;
  std::memcpy(flags, h->corpus.route.data() + first, (size_t)count);
  return MV_OK;
} catch (...) { return on_exception(h); }

int mv_corpus_row_forms(mv_handle* h, int64_t first, int64_t count, uint8_t* forms) try {
  if (!h || !forms) return fail(h, MV_ERR_INVALID, "mv_corpus_row_forms: bad argument");
  if (int rc = corpus_ready(h, CORPUS_ANY)) return rc;
  if (first < 0 || count <= 0 || first + count > h->corpus.n) return fail(h, MV_ERR_INVALID, "mv_corpus_row_forms: bad range");
  if (h->corpus.pending) return fail(h, MV_ERR_STATE, "mv_corpus_row_forms: a guarded sweep has not been collected yet (mv_corpus_results)");
  std::memcpy(forms, h->corpus.forms.data() + first, (size_t)count);
  return MV_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
