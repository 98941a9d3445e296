// libmemvul_retrieve.so: per-anchor retrieval over a kept corpus (include/memvul_retrieve.h; kernels and plan: report_topk.h).  A library of its own, which
// libmemvul_hip.so does not link against: the set of kernels in libmemvul_hip.so — what build.kernel_fingerprints hashes and tests/golden/pass_fingerprints.json is
// keyed on — and the list of mv_* entries both stay as they are.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/memvul_retrieve.h"
#include "report_topk.h"
#include "kept_index.h"

KEPT_ASSERT_ABI(MVR, MVR_MAX_QUERIES);

namespace {
const KeptKernels kReportKernels = {report_weight_delta_kernel, {report_row_term_kernel<512>, report_row_term_kernel<768>}, {report_query_prep_kernel<512>, report_query_prep_kernel<768>}};
}

struct mvr_index : KeptIndex {
  mvr_index() : KeptIndex(&kReportKernels, false, 2) {}
  // workspace (grows, never shrinks)
  float* list_p[2] = {nullptr, nullptr};  // candidate lists, ping and pong
  int32_t* list_row[2] = {nullptr, nullptr};
  size_t list_pn[2] = {0, 0}, list_rn[2] = {0, 0};
  float* top_p = nullptr;
  long long* top_row = nullptr;
  size_t top_pn = 0, top_rn = 0;
  float* ps = nullptr;                // mvr_psame's [count][Q]
  size_t ps_n = 0;
  int plan_block_rows = 0, plan_fan_in = 0, plan_anchor_group = 0;  // mvr_test_plan; 0 = the library's own choice
};

namespace {

struct Plan {
  int block_rows, fan_in, group;
  int64_t nblocks;
};

Plan plan_for(const mvr_index* h, int Q, int k, int64_t count) {
  Plan p;
  p.block_rows = h->plan_block_rows ? h->plan_block_rows : 256;
  p.fan_in = h->plan_fan_in ? h->plan_fan_in : 16;
  p.nblocks = (count + p.block_rows - 1) / p.block_rows;
  if (h->plan_anchor_group) {
    p.group = h->plan_anchor_group;
  } else {  // as many whole tiles as keep the lists within RT_LIST_CAP_BYTES, one at the least
    const int64_t per_q = std::max<int64_t>(p.nblocks, 1) * k * 8;
    const int64_t fit = RT_LIST_CAP_BYTES / per_q / RT_QT * RT_QT;
    p.group = (int)std::max<int64_t>(RT_QT, std::min<int64_t>(fit, (Q + RT_QT - 1) / RT_QT * RT_QT));
  }
  p.group = std::min(p.group, Q);
  return p;
}

template <int P, int PSAME>
void launch_score(mvr_index* h, int block_rows, dim3 grid, const ReportScoreArgs& a) {
  by_block_rows(block_rows, [&](auto br) {
    constexpr int BR = decltype(br)::value;
    hipLaunchKernelGGL((report_score_kernel<P, BR, PSAME>), grid, dim3(BR), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a);
  });
  launched("report_score_kernel");
}

// the group's vectors [q0, q0 + nq) transposed, its bv, then the score kernel over rows [first, first + count)
void score_group(mvr_index* h, const Plan& pl, int q0, int nq, int Q, int k, int64_t first, int64_t count, bool psame) {
  const int Qs = (nq + RT_QT - 1) / RT_QT * RT_QT;
  kept_vector_prep(h, q0, nq, Qs);
  ReportScoreArgs a{};
  a.first = first; a.count = count; a.nq = nq; a.Qs = Qs; a.same_idx = h->same_idx; a.k = k; a.nblocks = pl.nblocks;
  a.part_p = h->list_p[0]; a.part_row = h->list_row[0]; a.psame = h->ps; a.Q = Q; a.q0 = q0;
  const dim3 grid((unsigned)(Qs / RT_QT), (unsigned)std::min<int64_t>(pl.nblocks, RT_GRID_Y), (unsigned)((pl.nblocks + RT_GRID_Y - 1) / RT_GRID_Y));
  if (h->P == 512) { if (psame) launch_score<512, 1>(h, pl.block_rows, grid, a); else launch_score<512, 0>(h, pl.block_rows, grid, a); }
  else { if (psame) launch_score<768, 1>(h, pl.block_rows, grid, a); else launch_score<768, 0>(h, pl.block_rows, grid, a); }
}

// fold the group's lists until one is left; returns the number of launches
int merge_group(mvr_index* h, const Plan& pl, int q0, int nq, int k) {
  int64_t L = pl.nblocks;
  int src = 0, levels = 0;
  for (;;) {
    ReportMergeArgs m{};
    m.nq = nq; m.k = k; m.fan_in = pl.fan_in; m.L_in = L; m.L_out = (L + pl.fan_in - 1) / pl.fan_in; m.last = m.L_out == 1;
    m.in_p = h->list_p[src]; m.in_row = h->list_row[src]; m.out_p = h->list_p[1 - src]; m.out_row = h->list_row[1 - src];
    m.top_p = h->top_p; m.top_row = h->top_row; m.q0 = q0;
    const int64_t items = (int64_t)nq * m.L_out;
    const dim3 grid((unsigned)((items + 3) / 4)), block(256);
    const int n = (int)std::min<int64_t>(pl.fan_in, L) * k;
    if (n <= 64) hipLaunchKernelGGL(report_merge_kernel<1>, grid, block, 0, h->stream, m);
    else if (n <= 256) hipLaunchKernelGGL(report_merge_kernel<4>, grid, block, 0, h->stream, m);
    else hipLaunchKernelGGL(report_merge_kernel<16>, grid, block, 0, h->stream, m);
    launched("report_merge_kernel");
    ++levels;
    if (m.last) return levels;
    L = m.L_out;
    src = 1 - src;
  }
}

}  // namespace

extern "C" {

const char* mvr_last_error(mvr_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvr_create(int device, int proj_dim, const float* Wm, int same_idx, mvr_index** out) try {
  kept_create("retrieval index", mvr_destroy, device, proj_dim, Wm, same_idx, out);
  return MVR_OK;
} catch (...) { return on_exception(nullptr); }

void mvr_destroy(mvr_index* h) {
  if (!h) return;
  kept_destroy_common(h, {h->list_p[0], h->list_p[1], h->list_row[0], h->list_row[1], h->top_p, h->top_row, h->ps});
  delete h;
}

int mvr_add(mvr_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  kept_add(h, embed, n);
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_reset(mvr_index* h) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  h->n = 0;
  return MVR_OK;
} catch (...) { return on_exception(h); }

int64_t mvr_count(mvr_index* h) { return h ? h->n : 0; }

int mvr_query(mvr_index* h, const float* v, int Q, int k, int64_t first, int64_t count, float* top_p, int64_t* top_row) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  need(k >= 1 && k <= RT_KMAX, "k = " + std::to_string(k) + ": 1 <= k <= 64");
  check_range(h, "query vectors", v, Q, first, count);
  need(top_p != nullptr && top_row != nullptr, "an output buffer is NULL");
  h->timed = 0;
  const size_t out_n = (size_t)Q * k;
  if (count == 0) {  // nothing to rank: every slot is exhausted
    std::fill(top_p, top_p + out_n, -1.0f);
    std::fill(top_row, top_row + out_n, (int64_t)-1);
    return MVR_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const Plan pl = plan_for(h, Q, k, count);
  const int Qs = (pl.group + RT_QT - 1) / RT_QT * RT_QT;
  kept_upload_vectors(h, v, Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  const size_t l0 = (size_t)pl.group * pl.nblocks * k, l1 = (size_t)pl.group * ((pl.nblocks + pl.fan_in - 1) / pl.fan_in) * k;
  grow(h->list_p[0], h->list_pn[0], l0);
  grow(h->list_row[0], h->list_rn[0], l0);
  grow(h->list_p[1], h->list_pn[1], l1);
  grow(h->list_row[1], h->list_rn[1], l1);
  grow(h->top_p, h->top_pn, out_n);
  grow(h->top_row, h->top_rn, out_n);
  HIPCHK(hipEventRecord(h->ev[0], h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) {
    const int nq = std::min(pl.group, Q - q0);
    score_group(h, pl, q0, nq, Q, k, first, count, false);
    merge_group(h, pl, q0, nq, k);
  }
  HIPCHK(hipEventRecord(h->ev[1], h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = 1;
  HIPCHK(hipMemcpy(top_p, h->top_p, out_n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(top_row, h->top_row, out_n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_psame(mvr_index* h, const float* v, int Q, int64_t first, int64_t count, float* p) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  check_range(h, "query vectors", v, Q, first, count);
  need(count * (int64_t)Q <= MVR_MAX_PSAME, "count * Q = " + std::to_string(count * (int64_t)Q) + ": at most 2^28 values per call");
  need(p != nullptr || count == 0, "the output buffer is NULL");
  h->timed = 0;
  if (count == 0) return MVR_OK;
  HIPCHK(hipSetDevice(h->device));
  Plan pl = plan_for(h, Q, 1, count);
  if (!h->plan_anchor_group) pl.group = Q;  // (no lists to bound)
  const int Qs = (pl.group + RT_QT - 1) / RT_QT * RT_QT;
  kept_upload_vectors(h, v, Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  grow(h->ps, h->ps_n, (size_t)count * Q);
  HIPCHK(hipEventRecord(h->ev[0], h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) score_group(h, pl, q0, std::min(pl.group, Q - q0), Q, 1, first, count, true);
  HIPCHK(hipEventRecord(h->ev[1], h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = 1;
  HIPCHK(hipMemcpy(p, h->ps, (size_t)count * Q * sizeof(float), hipMemcpyDeviceToHost));
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_kernel_ms(mvr_index* h, float* ms) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  kept_kernel_ms(h, ms, "no query has launched a kernel yet");
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_test_plan(mvr_index* h, int block_rows, int fan_in, int anchor_group) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  check_block_rows(block_rows);
  need(fan_in == 0 || (fan_in >= 2 && fan_in <= 16), "fan_in = " + std::to_string(fan_in) + ": 0, or 2 .. 16 (fan_in * k <= 1024 candidates per wave)");
  need(anchor_group >= 0 && anchor_group <= MVR_MAX_QUERIES, "anchor_group = " + std::to_string(anchor_group) + ": 0 .. 4096");
  h->plan_block_rows = block_rows; h->plan_fan_in = fan_in; h->plan_anchor_group = anchor_group;
  return MVR_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
