// libmemvul_claims.so: per-anchor claims over a kept corpus (include/memvul_claims.h; kernels and plan: claim_sweep.h).  A library of its own, which no other
// library of this tree links against: their kernel sets, their source fingerprints and their lists of entries all stay as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/memvul_claims.h"
#include "claim_sweep.h"

struct mvc_index {
  int device = 0, P = 0, same_idx = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // ev[0..1] bracket the launches of a call; ev[2..3] those of mvc_select after its totals are known
  int timed = 0;                      // event pairs to add up
  float *U = nullptr, *sa = nullptr;  // rows [cap][P], row terms [cap]
  uint8_t* cls = nullptr;             // [cap]
  int64_t n = 0, cap = 0;
  float* wd = nullptr;                // [3][P] class-difference weights
  // workspace (grows, never shrinks)
  float *vdev = nullptr, *vT = nullptr, *bv = nullptr, *thr = nullptr;  // the vectors [Q][P]; one group transposed [P][Qs]; its bv [Qs]; the thresholds
  size_t vdev_n = 0, vT_n = 0, bv_n = 0, thr_n = 0;
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
  std::string err;
};

namespace {

thread_local std::string g_err;  // errors with no index to hang them on (mvc_create)

struct Refusal : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct StateError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(mvc_index* h, int code, const std::string& msg) {
  (h ? h->err : g_err) = msg;
  return code;
}

int on_exception(mvc_index* h) noexcept {
  try {
    try {
      throw;
    } catch (const Refusal& e) {
      return fail(h, MVC_ERR_ARG, e.what());
    } catch (const StateError& e) {
      return fail(h, MVC_ERR_STATE, e.what());
    } catch (const std::bad_alloc&) {
      return fail(h, MVC_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
      return fail(h, MVC_ERR_HIP, e.what());
    } catch (...) {
      return fail(h, MVC_ERR_INTERNAL, "unknown C++ exception");
    }
  } catch (...) {  // (the message itself could not be stored)
    return MVC_ERR_INTERNAL;
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

void reserve_rows(mvc_index* h, int64_t want) {
  if (want <= h->cap) return;
  const int64_t cap = std::max<int64_t>(want, std::min<int64_t>(h->cap + h->cap / 2, MVC_MAX_ROWS));
  float *U = nullptr, *sa = nullptr;
  uint8_t* cls = nullptr;
  hipError_t e = hipMalloc((void**)&U, (size_t)cap * h->P * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&sa, (size_t)cap * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&cls, (size_t)cap);
  if (e == hipSuccess && h->n) {
    e = hipMemcpyAsync(U, h->U, (size_t)h->n * h->P * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sa, h->sa, (size_t)h->n * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cls, h->cls, (size_t)h->n, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  if (e != hipSuccess) {
    for (void* p : {(void*)U, (void*)sa, (void*)cls})
      if (p) (void)hipFree(p);
    hipchk(e, "growing the rows' buffers");
  }
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->cls})
    if (p) (void)hipFree(p);
  h->U = U;
  h->sa = sa;
  h->cls = cls;
  h->cap = cap;
}

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
  switch (block_rows) {
    case 64: hipLaunchKernelGGL((claim_score_kernel<P, 64, MODE>), grid, dim3(64), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 128: hipLaunchKernelGGL((claim_score_kernel<P, 128, MODE>), grid, dim3(128), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 256: hipLaunchKernelGGL((claim_score_kernel<P, 256, MODE>), grid, dim3(256), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    default: hipLaunchKernelGGL((claim_score_kernel<P, 512, MODE>), grid, dim3(512), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
  }
  launched("claim_score_kernel");
}

// the group's vectors [q0, q0 + nq) transposed and their bv (skipped when the last prep was this group's), then the score kernel over rows [first, first + count)
void score_group(mvc_index* h, const Plan& pl, int mode, int q0, int nq, bool prep, ClaimScoreArgs a) {
  const int Qs = (nq + CL_QT - 1) / CL_QT * CL_QT;
  if (prep) {
    const float* v = h->vdev + (size_t)q0 * h->P;
    if (h->P == 512) hipLaunchKernelGGL(claim_vector_prep_kernel<512>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, v, h->wd, h->vT, h->bv, nq, Qs);
    else hipLaunchKernelGGL(claim_vector_prep_kernel<768>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, v, h->wd, h->vT, h->bv, nq, Qs);
    launched("claim_vector_prep_kernel");
  }
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

void check_range(const mvc_index* h, const float* v, int Q, int64_t first, int64_t count) {
  need(v != nullptr, "the vectors are NULL");
  need(Q >= 1 && Q <= MVC_MAX_VECTORS, "Q = " + std::to_string(Q) + ": 1 <= Q <= 4096");
  need(first >= 0 && count >= 0 && first <= h->n && count <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not within the " + std::to_string(h->n) + " rows of the index");
}

void check_thresholds(const float* thres, int n) {
  need(thres != nullptr, "the thresholds are NULL");
  for (int i = 0; i < n; ++i) need(std::isfinite(thres[i]), "thres[" + std::to_string(i) + "] is not finite");
}

void upload(mvc_index* h, const float* v, int Q, const float* thres, int nthr) {
  grow(h->vdev, h->vdev_n, (size_t)Q * h->P);
  grow(h->thr, h->thr_n, (size_t)nthr);
  HIPCHK(hipMemcpyAsync(h->vdev, v, (size_t)Q * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
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
  need(out != nullptr, "out is NULL");
  *out = nullptr;
  need(proj_dim == 512 || proj_dim == 768, "proj_dim = " + std::to_string(proj_dim) + ": the matcher runs on 512 or 768 features");
  need(same_idx == 0 || same_idx == 1, "same_idx = " + std::to_string(same_idx) + ": 0 or 1");
  need(Wm != nullptr, "the matcher weight is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MVC_ERR_HIP, "no HIP device: the claim index has no CPU fallback");
  need(device >= 0 && device < ndev, "device " + std::to_string(device) + " of " + std::to_string(ndev));
  HIPCHK(hipSetDevice(device));
  mvc_index* h = new mvc_index();
  h->device = device; h->P = proj_dim; h->same_idx = same_idx;
  try {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev) HIPCHK(hipEventCreate(&e));
    float* wm = nullptr;
    HIPCHK(hipMalloc((void**)&h->wd, (size_t)3 * h->P * sizeof(float)));
    HIPCHK(hipMalloc((void**)&wm, (size_t)6 * h->P * sizeof(float)));
    hipError_t e = hipMemcpyAsync(wm, Wm, (size_t)6 * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(claim_weight_delta_kernel, dim3((3 * h->P + 255) / 256), dim3(256), 0, h->stream, wm, h->wd, h->P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(wm);
    hipchk(e, "uploading the matcher weight");
  } catch (...) {
    mvc_destroy(h);
    throw;
  }
  *out = h;
  return MVC_OK;
} catch (...) { return on_exception(nullptr); }

void mvc_destroy(mvc_index* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->cls, (void*)h->wd, (void*)h->vdev, (void*)h->vT, (void*)h->bv, (void*)h->thr, (void*)h->part, (void*)h->counts,
                  (void*)h->bits, (void*)h->wbase, (void*)h->totals, (void*)h->offs, (void*)h->sel_rows, (void*)h->sel_p})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int mvc_add(mvc_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  need(n >= 0, "n = " + std::to_string(n) + " rows");
  need(n <= MVC_MAX_ROWS - h->n, "the index would hold more than 2^31 - 2 rows");
  if (n == 0) return MVC_OK;
  need(embed != nullptr, "the embeddings are NULL");
  HIPCHK(hipSetDevice(h->device));
  reserve_rows(h, h->n + n);
  HIPCHK(hipMemcpyAsync(h->U + (size_t)h->n * h->P, embed, (size_t)n * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->cls + h->n, 0, (size_t)n, h->stream));
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (h->P == 512) hipLaunchKernelGGL(claim_row_term_kernel<512>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  else hipLaunchKernelGGL(claim_row_term_kernel<768>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  launched("claim_row_term_kernel");
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's buffer is free again, and the rows count only once they are there)
  h->n += n;
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
  need(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  if (n == 0) return MVC_OK;
  need(cls != nullptr, "the classes are NULL");
  for (int64_t i = 0; i < n; ++i) need(cls[i] <= 1, "cls[" + std::to_string(i) + "] = " + std::to_string((int)cls[i]) + ": a class is 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->cls + first, cls, (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_counts(mvc_index* h, const float* v, int Q, const float* thres, int T, int64_t first, int64_t count, int64_t* counts) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  h->timed = 0;
  need(T >= 1 && T <= MVC_MAX_THRESHOLDS, "T = " + std::to_string(T) + ": 1 <= T <= 64");
  check_range(h, v, Q, first, count);
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
  check_range(h, v, Q, first, count);
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
  need(ms != nullptr, "ms is NULL");
  need(h->timed > 0, "no call has launched a kernel yet");
  float a = 0.f, b = 0.f;
  HIPCHK(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  if (h->timed > 1) HIPCHK(hipEventElapsedTime(&b, h->ev[2], h->ev[3]));
  *ms = a + b;
  return MVC_OK;
} catch (...) { return on_exception(h); }

int mvc_test_plan(mvc_index* h, int block_rows, int vector_group) try {
  if (!h) return fail(nullptr, MVC_ERR_ARG, "index is NULL");
  drop_selection(h);
  need(block_rows == 0 || block_rows == 64 || block_rows == 128 || block_rows == 256 || block_rows == 512,
       "block_rows = " + std::to_string(block_rows) + ": 0, 64, 128, 256 or 512");
  need(vector_group >= 0 && vector_group <= MVC_MAX_VECTORS, "vector_group = " + std::to_string(vector_group) + ": 0 .. 4096");
  h->plan_block_rows = block_rows; h->plan_vector_group = vector_group;
  return MVC_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
