// libmemvul_retrieve.so: per-anchor retrieval over a kept corpus (include/memvul_retrieve.h; kernels and plan: report_topk.h).  A library of its own, which
// libmemvul_hip.so does not link against: the set of kernels in libmemvul_hip.so — what build.kernel_fingerprints hashes and tests/golden/pass_fingerprints.json is
// keyed on — and the list of mv_* entries both stay as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/memvul_retrieve.h"
#include "report_topk.h"

struct mvr_index {
  int device = 0, P = 0, same_idx = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;                 // ev0 / ev1 bracket the launches of a query
  float *U = nullptr, *sa = nullptr;  // rows [cap][P], row terms [cap]
  int64_t n = 0, cap = 0;
  float* wd = nullptr;                // [3][P] class-difference weights
  // workspace (grows, never shrinks)
  float *vdev = nullptr, *vT = nullptr, *bv = nullptr;  // the query vectors [Q][P]; one group transposed [P][Qs]; its bv [Qs]
  size_t vdev_n = 0, vT_n = 0, bv_n = 0;
  float* list_p[2] = {nullptr, nullptr};  // candidate lists, ping and pong
  int32_t* list_row[2] = {nullptr, nullptr};
  size_t list_pn[2] = {0, 0}, list_rn[2] = {0, 0};
  float* top_p = nullptr;
  long long* top_row = nullptr;
  size_t top_pn = 0, top_rn = 0;
  float* ps = nullptr;                // mvr_psame's [count][Q]
  size_t ps_n = 0;
  int plan_block_rows = 0, plan_fan_in = 0, plan_anchor_group = 0;  // mvr_test_plan; 0 = the library's own choice
  std::string err;
};

namespace {

thread_local std::string g_err;  // errors with no index to hang them on (mvr_create)

struct Refusal : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(mvr_index* h, int code, const std::string& msg) {
  (h ? h->err : g_err) = msg;
  return code;
}

int on_exception(mvr_index* h) noexcept {
  try {
    try {
      throw;
    } catch (const Refusal& e) {
      return fail(h, MVR_ERR_ARG, e.what());
    } catch (const std::bad_alloc&) {
      return fail(h, MVR_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
      return fail(h, MVR_ERR_HIP, e.what());
    } catch (...) {
      return fail(h, MVR_ERR_INTERNAL, "unknown C++ exception");
    }
  } catch (...) {  // (the message itself could not be stored)
    return MVR_ERR_INTERNAL;
  }
}

void hipchk(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(X) hipchk((X), #X)

void launched(const char* what) { hipchk(hipGetLastError(), what); }

void need(bool ok, const std::string& msg) {
  if (!ok) throw Refusal(msg);
}

template <typename T>
void grow(T*& p, size_t& have, size_t want) {  // (contents are not kept)
  if (want <= have) return;
  if (p) HIPCHK(hipFree(p));
  p = nullptr;
  have = 0;
  HIPCHK(hipMalloc((void**)&p, want * sizeof(T)));
  have = want;
}

void reserve_rows(mvr_index* h, int64_t want) {
  if (want <= h->cap) return;
  const int64_t cap = std::max<int64_t>(want, std::min<int64_t>(h->cap + h->cap / 2, MVR_MAX_ROWS));
  float *U = nullptr, *sa = nullptr;
  HIPCHK(hipMalloc((void**)&U, (size_t)cap * h->P * sizeof(float)));
  if (hipMalloc((void**)&sa, (size_t)cap * sizeof(float)) != hipSuccess) {
    (void)hipFree(U);
    throw std::runtime_error("hipMalloc of the row terms failed");
  }
  if (h->n) {
    hipError_t e = hipMemcpyAsync(U, h->U, (size_t)h->n * h->P * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sa, h->sa, (size_t)h->n * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      (void)hipFree(U);
      (void)hipFree(sa);
      hipchk(e, "copying the rows to their larger buffer");
    }
  }
  if (h->U) (void)hipFree(h->U);
  if (h->sa) (void)hipFree(h->sa);
  h->U = U;
  h->sa = sa;
  h->cap = cap;
}

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
  switch (block_rows) {
    case 64: hipLaunchKernelGGL((report_score_kernel<P, 64, PSAME>), grid, dim3(64), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 128: hipLaunchKernelGGL((report_score_kernel<P, 128, PSAME>), grid, dim3(128), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 256: hipLaunchKernelGGL((report_score_kernel<P, 256, PSAME>), grid, dim3(256), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    default: hipLaunchKernelGGL((report_score_kernel<P, 512, PSAME>), grid, dim3(512), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
  }
  launched("report_score_kernel");
}

// the group's vectors [q0, q0 + nq) transposed, its bv, then the score kernel over rows [first, first + count)
void score_group(mvr_index* h, const Plan& pl, int q0, int nq, int Q, int k, int64_t first, int64_t count, bool psame) {
  const int Qs = (nq + RT_QT - 1) / RT_QT * RT_QT;
  const float* v = h->vdev + (size_t)q0 * h->P;
  if (h->P == 512) hipLaunchKernelGGL(report_query_prep_kernel<512>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, v, h->wd, h->vT, h->bv, nq, Qs);
  else hipLaunchKernelGGL(report_query_prep_kernel<768>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, v, h->wd, h->vT, h->bv, nq, Qs);
  launched("report_query_prep_kernel");
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

void check_range(const mvr_index* h, const float* v, int Q, int64_t first, int64_t count) {
  need(v != nullptr, "the query vectors are NULL");
  need(Q >= 1 && Q <= MVR_MAX_QUERIES, "Q = " + std::to_string(Q) + ": 1 <= Q <= 4096");
  need(first >= 0 && count >= 0 && first <= h->n && count <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not within the " + std::to_string(h->n) + " rows of the index");
}

void upload_queries(mvr_index* h, const float* v, int Q) {
  grow(h->vdev, h->vdev_n, (size_t)Q * h->P);
  HIPCHK(hipMemcpyAsync(h->vdev, v, (size_t)Q * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
}

}  // namespace

extern "C" {

const char* mvr_last_error(mvr_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvr_create(int device, int proj_dim, const float* Wm, int same_idx, mvr_index** out) try {
  need(out != nullptr, "out is NULL");
  *out = nullptr;
  need(proj_dim == 512 || proj_dim == 768, "proj_dim = " + std::to_string(proj_dim) + ": the matcher runs on 512 or 768 features");
  need(same_idx == 0 || same_idx == 1, "same_idx = " + std::to_string(same_idx) + ": 0 or 1");
  need(Wm != nullptr, "the matcher weight is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MVR_ERR_HIP, "no HIP device: the retrieval index has no CPU fallback");
  need(device >= 0 && device < ndev, "device " + std::to_string(device) + " of " + std::to_string(ndev));
  HIPCHK(hipSetDevice(device));
  mvr_index* h = new mvr_index();
  h->device = device; h->P = proj_dim; h->same_idx = same_idx;
  try {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    float* wm = nullptr;
    HIPCHK(hipMalloc((void**)&h->wd, (size_t)3 * h->P * sizeof(float)));
    HIPCHK(hipMalloc((void**)&wm, (size_t)6 * h->P * sizeof(float)));
    hipError_t e = hipMemcpyAsync(wm, Wm, (size_t)6 * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(report_weight_delta_kernel, dim3((3 * h->P + 255) / 256), dim3(256), 0, h->stream, wm, h->wd, h->P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(wm);
    hipchk(e, "uploading the matcher weight");
  } catch (...) {
    mvr_destroy(h);
    throw;
  }
  *out = h;
  return MVR_OK;
} catch (...) { return on_exception(nullptr); }

void mvr_destroy(mvr_index* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->wd, (void*)h->vdev, (void*)h->vT, (void*)h->bv, (void*)h->list_p[0], (void*)h->list_p[1],
                  (void*)h->list_row[0], (void*)h->list_row[1], (void*)h->top_p, (void*)h->top_row, (void*)h->ps})
    if (p) (void)hipFree(p);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int mvr_add(mvr_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  need(n >= 0, "n = " + std::to_string(n) + " rows");
  need(n <= MVR_MAX_ROWS - h->n, "the index would hold more than 2^31 - 2 rows");
  if (n == 0) return MVR_OK;
  need(embed != nullptr, "the embeddings are NULL");
  HIPCHK(hipSetDevice(h->device));
  reserve_rows(h, h->n + n);
  HIPCHK(hipMemcpyAsync(h->U + (size_t)h->n * h->P, embed, (size_t)n * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (h->P == 512) hipLaunchKernelGGL(report_row_term_kernel<512>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  else hipLaunchKernelGGL(report_row_term_kernel<768>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  launched("report_row_term_kernel");
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's buffer is free again, and the rows count only once they are there)
  h->n += n;
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
  check_range(h, v, Q, first, count);
  need(top_p != nullptr && top_row != nullptr, "an output buffer is NULL");
  h->timed = false;
  const size_t out_n = (size_t)Q * k;
  if (count == 0) {  // nothing to rank: every slot is exhausted
    std::fill(top_p, top_p + out_n, -1.0f);
    std::fill(top_row, top_row + out_n, (int64_t)-1);
    return MVR_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const Plan pl = plan_for(h, Q, k, count);
  const int Qs = (pl.group + RT_QT - 1) / RT_QT * RT_QT;
  upload_queries(h, v, Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  const size_t l0 = (size_t)pl.group * pl.nblocks * k, l1 = (size_t)pl.group * ((pl.nblocks + pl.fan_in - 1) / pl.fan_in) * k;
  grow(h->list_p[0], h->list_pn[0], l0);
  grow(h->list_row[0], h->list_rn[0], l0);
  grow(h->list_p[1], h->list_pn[1], l1);
  grow(h->list_row[1], h->list_rn[1], l1);
  grow(h->top_p, h->top_pn, out_n);
  grow(h->top_row, h->top_rn, out_n);
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) {
    const int nq = std::min(pl.group, Q - q0);
    score_group(h, pl, q0, nq, Q, k, first, count, false);
    merge_group(h, pl, q0, nq, k);
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = true;
  HIPCHK(hipMemcpy(top_p, h->top_p, out_n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(top_row, h->top_row, out_n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_psame(mvr_index* h, const float* v, int Q, int64_t first, int64_t count, float* p) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  check_range(h, v, Q, first, count);
  need(count * (int64_t)Q <= MVR_MAX_PSAME, "count * Q = " + std::to_string(count * (int64_t)Q) + ": at most 2^28 values per call");
  need(p != nullptr || count == 0, "the output buffer is NULL");
  h->timed = false;
  if (count == 0) return MVR_OK;
  HIPCHK(hipSetDevice(h->device));
  Plan pl = plan_for(h, Q, 1, count);
  if (!h->plan_anchor_group) pl.group = Q;  // (no lists to bound)
  const int Qs = (pl.group + RT_QT - 1) / RT_QT * RT_QT;
  upload_queries(h, v, Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, (size_t)Qs);
  grow(h->ps, h->ps_n, (size_t)count * Q);
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int q0 = 0; q0 < Q; q0 += pl.group) score_group(h, pl, q0, std::min(pl.group, Q - q0), Q, 1, first, count, true);
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->timed = true;
  HIPCHK(hipMemcpy(p, h->ps, (size_t)count * Q * sizeof(float), hipMemcpyDeviceToHost));
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_kernel_ms(mvr_index* h, float* ms) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  need(ms != nullptr, "ms is NULL");
  need(h->timed, "no query has launched a kernel yet");
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return MVR_OK;
} catch (...) { return on_exception(h); }

int mvr_test_plan(mvr_index* h, int block_rows, int fan_in, int anchor_group) try {
  if (!h) return fail(nullptr, MVR_ERR_ARG, "index is NULL");
  need(block_rows == 0 || block_rows == 64 || block_rows == 128 || block_rows == 256 || block_rows == 512,
       "block_rows = " + std::to_string(block_rows) + ": 0, 64, 128, 256 or 512");
  need(fan_in == 0 || (fan_in >= 2 && fan_in <= 16), "fan_in = " + std::to_string(fan_in) + ": 0, or 2 .. 16 (fan_in * k <= 1024 candidates per wave)");
  need(anchor_group >= 0 && anchor_group <= MVR_MAX_QUERIES, "anchor_group = " + std::to_string(anchor_group) + ": 0 .. 4096");
  h->plan_block_rows = block_rows; h->plan_fan_in = fan_in; h->plan_anchor_group = anchor_group;
  return MVR_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
