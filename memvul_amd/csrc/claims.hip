// libmemvul_claims.so: per-anchor claims over a kept corpus (include/memvul_claims.h; kernels and plan: claim_sweep.h).  A library of its own, which no other
// library of this tree links against: their kernel sets, their source fingerprints and their lists of entries all stay as they are.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/memvul_claims.h"
#include "claim_sweep.h"
#include "kept_index.h"

KEPT_ASSERT_ABI(MVC, MVC_MAX_VECTORS);
static_assert(MVC_ERR_STATE == KEPT_ERR_STATE, "the public header and kept_index.h disagree");

namespace {
const KeptKernels kClaimKernels = {claim_weight_delta_kernel, {claim_row_term_kernel<512>, claim_row_term_kernel<768>}, {claim_vector_prep_kernel<512>, claim_vector_prep_kernel<768>}};
}

struct mvc_index : KeptIndex {
  mvc_index() : KeptIndex(&kClaimKernels, true, 4) {}  // (ev[2..3]: the launches of mvc_select after its totals are known)
  // workspace (grows, never shrinks)
  float* thr = nullptr;               // the thresholds
  size_t thr_n = 0;
  uint32_t* part = nullptr;           // mvc_counts: partials [group][blocks][T]
  long long* counts = nullptr;        // [Q][T][2]
  size_t part_n = 0, counts_n = 0;
  unsigned long long* bits = nullptr; // mvc_select: [group][W]
  uint32_t* wbase = nullptr;          // [group][W]
  long long *totals = nullptr, *offs = nullptr;  // [Q], [Q + 1]
  size_t bits_n = 0, wbase_n = 0, totals_n = 0, offs_n = 0;
  // the held selection
  bool held = false;
  int64_t sel_total = 0;
  long long* sel_rows = nullptr;
  float* sel_p = nullptr;
  size_t sel_rows_n = 0, sel_p_n = 0;
  int plan_block_rows = 0, plan_vector_group = 0;  // mvc_test_plan; 0 = the library's own choice
};

namespace {

struct Plan {
  int block_rows, group;
  int64_t nblocks, W;
};

// per_vector: the workspace bytes one vector of a group costs
Plan plan_for(const mvc_index* h, int Q, int64_t count, int64_t per_block_bytes, int64_t per_word_bytes) {
  Plan p;
  p.block_rows = h->plan_block_rows ? h->plan_block_rows : 256;
  p.nblocks = (count + p.block_rows - 1) / p.block_rows;
  p.W = (count + 63) / 64;
  if (h->plan_vector_group) {
    p.group = h->plan_vector_group;
  } else {  // as many whole tiles as keep the group's workspace within CL_WORK_CAP_BYTES, one at the least
    const int64_t per_q = std::max<int64_t>(p.nblocks * per_block_bytes + p.W * per_word_bytes, 1);
    const int64_t fit = CL_WORK_CAP_BYTES / per_q / CL_QT * CL_QT;
    p.group = (int)std::max<int64_t>(CL_QT, std::min<int64_t>(fit, (Q + CL_QT - 1) / CL_QT * CL_QT));
  }
  p.group = std::min(p.group, Q);
  return p;
}

template <int P, int MODE>
void launch_score(mvc_index* h, int block_rows, dim3 grid, const ClaimScoreArgs& a) {
  by_block_rows(block_rows, [&](auto br) {
    constexpr int BR = decltype(br)::value;
    hipLaunchKernelGGL((claim_score_kernel<P, BR, MODE>), grid, dim3(BR), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a);
  });
  launched("claim_score_kernel");
}

// the group's vectors [q0, q0 + nq) transposed and their bv (skipped when the last prep was this group's), then the score kernel over rows [first, first + count)
void score_group(mvc_index* h, const Plan& pl, int mode, int q0, int nq, bool prep, ClaimScoreArgs a) {
  const int Qs = (nq + CL_QT - 1) / CL_QT * CL_QT;
  if (prep) kept_vector_prep(h, q0, nq, Qs);
  a.nq = nq; a.Qs = Qs; a.q0 = q0; a.same_idx = h->same_idx; a.nblocks = pl.nblocks; a.W = pl.W;
  a.thr = h->thr; a.cls = h->cls; a.part = h->part; a.bits = h->bits; a.wbase = h->wbase; a.offs = h->offs; a.rows = h->sel_rows; a.p = h->sel_p;
  const dim3 grid((unsigned)(Qs / CL_QT), (unsigned)std::min<int64_t>(pl.nblocks, CL_GRID_Y), (unsigned)((pl.nblocks + CL_GRID_Y - 1) / CL_GRID_Y));
  if (h->P == 512) {
    if (mode == CL_COUNT) launch_score<512, CL_COUNT>(h, pl.block_rows, grid, a);
    else if (mode == CL_MARK) launch_score<512, CL_MARK>(h, pl.block_rows, grid, a);
    else launch_score<512, CL_FILL>(h, pl.block_rows, grid, a);
  } else {
    if (mode == CL_COUNT) launch_score<768, CL_COUNT>(h, pl.block_rows, grid, a);
    else if (mode == CL_MARK) launch_score<768, CL_MARK>(h, pl.block_rows, grid, a);
    else launch_score<768, CL_FILL>(h, pl.block_rows, grid, a);
  }
}

// CL_MARK over the group, then the scan of its words
void mark_group(mvc_index* h, const Plan& pl, int q0, int nq, const ClaimScoreArgs& a) {
  score_group(h, pl, CL_MARK, q0, nq, true, a);
  hipLaunchKernelGGL(claim_scan_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream, h->bits, h->wbase, h->totals, (long long)pl.W, q0);
  launched("claim_scan_kernel");
}

void upload(mvc_index* h, const float* v, int Q, const float* thres, int nthr) {
  grow(h->thr, h->thr_n, (size_t)nthr);
  kept_upload_vectors(h, v, Q);
  HIPCHK(hipMemcpyAsync(h->thr, thres, (size_t)nthr * sizeof(float), hipMemcpyHostToDevice, h->stream));
}

void drop_selection(mvc_index* h) {
  h->held = false;
  h->sel_total = 0;
}

}  // namespace

extern "C" {

const char* mvc_last_error(mvc_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvc_create(int device, int proj_dim, const float* Wm, int same_idx, mvc_index** out) try {
  kept_create("claim index", mvc_destroy, device, proj_dim, Wm, same_idx, out);
  return MVC_OK;
} catch (...) { return on_exception(nullptr); }

void mvc_destroy(mvc_index* h) {
  if (!h) return;
  kept_destroy_common(h, {h->thr, h->part, h->counts, h->bits, h->wbase, h->totals, h->offs, h->sel_rows, h->sel_p});
  delete h;
}

int mvc_add(mvc_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  kept_add(h, embed, n);
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_reset(mvc_index* h) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  h->n = 0;
  return MVC_OK;
} catch (...) { return on_exception(h); }

int64_t mvc_count(mvc_index* h) { return h ? h->n : 0; }

int mvc_set_classes(mvc_index* h, const uint8_t* cls, int64_t first, int64_t n) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  kept_set_classes(h, cls, first, n);
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_counts(mvc_index* h, const float* v, int Q, const float* thres, int T, int64_t first, int64_t count, int64_t* counts) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  h->timed = 0;
  need(T >= 1 && T <= MVC_MAX_THRESHOLDS, "T = " + std::to_string(T) + ": 1 <= T <= 64");
  check_range(h, "vectors", v, Q, first, count);
  check_thresholds(thres, T);
  need(counts != nullptr, "the output buffer is NULL");
  const size_t out_n = (size_t)Q * T * 2;
  if (count == 0) {
    std::fill(counts, counts + out_n, (int64_t)0);
    return MVC_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const Plan pl = plan_for(h, Q, count, (int64_t)T * 4, 0);
  const int Qs = (pl.group + CL_QT - 1) / CL_QT * CL_QT;
  upload(h, v, Q, thres, T);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  grow(h->part, h->part_n, (size_t)pl.group * pl.nblocks * T);
  grow(h->counts, h->counts_n, out_n);
  ClaimScoreArgs a{};
  a.first = first; a.count = count; a.T = T;
  HIPCHK(hipEventRecord(h->ev[0], h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) {
    const int nq = std::min(pl.group, Q - q0);
    score_group(h, pl, CL_COUNT, q0, nq, true, a);
    hipLaunchKernelGGL(claim_fold_kernel, dim3((unsigned)nq), dim3(64 * CL_FOLD_WAVES), 0, h->stream, h->part, h->counts, (long long)pl.nblocks, T, q0);
    launched("claim_fold_kernel");
  }
  HIPCHK(hipEventRecord(h->ev[1], h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = 1;
  static_assert(sizeof(long long) == sizeof(int64_t), "counts are copied as they are");
  HIPCHK(hipMemcpy(counts, h->counts, out_n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_select(mvc_index* h, const float* v, int Q, const float* thres, int64_t first, int64_t count, int64_t* offsets) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  h->timed = 0;
  check_range(h, "vectors", v, Q, first, count);
  check_thresholds(thres, Q);
  need(offsets != nullptr, "the output buffer is NULL");
  if (count == 0) {  // nothing to claim: an empty selection is held
    std::fill(offsets, offsets + Q + 1, (int64_t)0);
    h->held = true;
    return MVC_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const Plan pl = plan_for(h, Q, count, 0, 12);
  const int Qs = (pl.group + CL_QT - 1) / CL_QT * CL_QT;
  const bool one_group = pl.group >= Q;
  upload(h, v, Q, thres, Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  grow(h->bits, h->bits_n, (size_t)pl.group * pl.W);
  grow(h->wbase, h->wbase_n, (size_t)pl.group * pl.W);
  grow(h->totals, h->totals_n, (size_t)Q);
  grow(h->offs, h->offs_n, (size_t)Q + 1);
  ClaimScoreArgs a{};
  a.first = first; a.count = count;
  // 1: mark and scan every group; the totals say how much the survivors need
  HIPCHK(hipEventRecord(h->ev[0], h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) mark_group(h, pl, q0, std::min(pl.group, Q - q0), a);
  HIPCHK(hipEventRecord(h->ev[1], h->stream));
  std::vector<long long> offs((size_t)Q + 1, 0);
  HIPCHK(hipMemcpyAsync(offs.data() + 1, h->totals, (size_t)Q * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = 1;
  for (int q = 0; q < Q; ++q) offs[q + 1] += offs[q];
  const long long total = offs[Q];
  need(total <= MVC_MAX_PAIRS, "the selection holds " + std::to_string(total) + " pairs: at most 2^28 per call (raise the thresholds, or select fewer vectors or rows)");
  // 2: the survivors, sized from the scan; a single group's words are still there, several groups are marked again one by one
  if (total > 0) {
    grow(h->sel_rows, h->sel_rows_n, (size_t)total);
    grow(h->sel_p, h->sel_p_n, (size_t)total);
    HIPCHK(hipMemcpyAsync(h->offs, offs.data(), ((size_t)Q + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    a.total = total;
    HIPCHK(hipEventRecord(h->ev[2], h->stream));
    for (int q0 = 0; q0 < Q; q0 += pl.group) {
      const int nq = std::min(pl.group, Q - q0);
      if (!one_group) mark_group(h, pl, q0, nq, a);
      score_group(h, pl, CL_FILL, q0, nq, false, a);
    }
    HIPCHK(hipEventRecord(h->ev[3], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timed = 2;
  }
  std::copy(offs.begin(), offs.end(), offsets);
  h->sel_total = total;
  h->held = true;
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_fetch(mvc_index* h, int64_t* rows, float* p) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  if (!h->held) throw StateError("no selection is held: mvc_fetch follows a successful mvc_select, with no other call on the index in between");
  if (h->sel_total == 0) return MVC_OK;
  need(rows != nullptr && p != nullptr, "an output buffer is NULL");
  HIPCHK(hipSetDevice(h->device));
  // (both copies land or neither is reported: the first goes to a buffer of the library's own)
  std::vector<int64_t> r((size_t)h->sel_total);
  HIPCHK(hipMemcpy(r.data(), h->sel_rows, (size_t)h->sel_total * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(p, h->sel_p, (size_t)h->sel_total * sizeof(float), hipMemcpyDeviceToHost));
  std::copy(r.begin(), r.end(), rows);
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_kernel_ms(mvc_index* h, float* ms) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  kept_kernel_ms(h, ms, "no call has launched a kernel yet");
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_test_plan(mvc_index* h, int block_rows, int vector_group) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  check_block_rows(block_rows);
  need(vector_group >= 0 && vector_group <= MVC_MAX_VECTORS, "vector_group = " + std::to_string(vector_group) + ": 0 .. 4096");
  h->plan_block_rows = block_rows; h->plan_vector_group = vector_group;
  return MVC_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
