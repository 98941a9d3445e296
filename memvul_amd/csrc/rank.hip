// libmemvul_rank.so: per-anchor ranking quality over a kept corpus (include/memvul_rank.h; kernels and plan: rank_sort.h).  A library of its own, which no other
// library of this tree links against and which includes no file of theirs: their kernel sets, their source fingerprints and their lists of entries all stay as
// they are.  The host side of an index over a kept corpus (the rows and their row terms on the device, the error plumbing of the C boundary, create / add /
// set_classes / kernel_ms) is therefore restated here.  Everything but the entries has INTERNAL linkage: a process loads the side libraries next to each other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/memvul_rank.h"
#include "rank_sort.h"

struct mvk_index {
  int device = 0, P = 0, same_idx = 0;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;         // the stage boundaries of a call, in order; created as needed, kept
  std::vector<int> ev_stage;          // the stage that ends at each event of the last call (-1: none)
  float ms[4] = {0.f, 0.f, 0.f, 0.f}; // the last call: whole, score, sort, statistics
  bool timed = false;
  float *U = nullptr, *sa = nullptr;  // rows [cap][P], row terms [cap]
  uint8_t* cls = nullptr;             // [cap]
  int64_t n = 0, cap = 0;
  float* wd = nullptr;                // [3][P] class-difference weights
  // workspace (grows, never shrinks)
  float *vdev = nullptr, *vT = nullptr, *bv = nullptr;  // the vectors [Q][P]; one group transposed [P][Qs]; its bv [Qs]
  size_t vdev_n = 0, vT_n = 0, bv_n = 0;
  uint32_t *keys_a = nullptr, *keys_b = nullptr, *hist = nullptr, *bank = nullptr;  // [group][count] twice; [group][ntiles][256]; [count]
  size_t keys_a_n = 0, keys_b_n = 0, hist_n = 0, bank_n = 0;
  RankTileSum* sums = nullptr;        // [group][ntiles]
  RankTileCarry* carry = nullptr;
  RankTotals* totals = nullptr;       // [group]
  long long* p_u2 = nullptr;          // [group][ntiles]
  double* p_ap = nullptr;             // [group][nchunks]
  RankBest* p_best = nullptr;         // [group][ntiles]
  size_t sums_n = 0, carry_n = 0, totals_n = 0, p_u2_n = 0, p_ap_n = 0, p_best_n = 0;
  long long *o_n = nullptr, *o_u2 = nullptr, *o_best = nullptr;  // the result slots
  double* o_ap = nullptr;
  float* o_thres = nullptr;
  size_t o_n_n = 0, o_u2_n = 0, o_best_n = 0, o_ap_n = 0, o_thres_n = 0;
  // the held curve
  bool held = false;
  int64_t points = 0;
  float* c_thres = nullptr;
  long long *c_tp = nullptr, *c_fp = nullptr;
  size_t c_thres_n = 0, c_tp_n = 0, c_fp_n = 0;
  int plan_tile_rows = 0, plan_vector_group = 0;  // mvk_test_plan; 0 = the library's own choice
  int64_t plan_work_cap = 0;
  std::string err;
};

namespace {

thread_local std::string g_err;  // errors with no index to hang them on (create)

struct Refusal : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct StateError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(mvk_index* h, int code, const std::string& msg) {
  (h ? h->err : g_err) = msg;
  return code;
}

int on_exception(mvk_index* h) noexcept {
  try {
    try {
      throw;
    } catch (const Refusal& e) {
      return fail(h, MVK_ERR_ARG, e.what());
    } catch (const StateError& e) {
      return fail(h, MVK_ERR_STATE, e.what());
    } catch (const std::bad_alloc&) {
      return fail(h, MVK_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
      return fail(h, MVK_ERR_HIP, e.what());
    } catch (...) {
      return fail(h, MVK_ERR_INTERNAL, "unknown C++ exception");
    }
  } catch (...) {  // (the message itself could not be stored)
    return MVK_ERR_INTERNAL;
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

void reserve_rows(mvk_index* h, int64_t want) {
  if (want <= h->cap) return;
  const int64_t cap = std::max<int64_t>(want, std::min<int64_t>(h->cap + h->cap / 2, MVK_MAX_ROWS));
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

void drop_curve(mvk_index* h) {
  h->held = false;
  h->points = 0;
}

void check_range(const mvk_index* h, const float* v, int Q, int64_t first, int64_t count) {
  need(v != nullptr, "the vectors are NULL");
  need(Q >= 1 && Q <= MVK_MAX_VECTORS, "Q = " + std::to_string(Q) + ": 1 <= Q <= 4096");
  need(first >= 0 && count >= 0 && first <= h->n && count <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  need(count <= MVK_MAX_RANK_ROWS, "count = " + std::to_string(count) + ": one call ranks at most 2^26 rows (MVK_MAX_RANK_ROWS)");
}

// ---- the plan

struct Plan {
  int tile, group;       // rows per sort tile; vectors per group
  int ntiles, nchunks;
};

// the workspace bytes one vector of a group costs over `count` rows in tiles of `tile`
int64_t vector_bytes(int64_t count, int tile) {
  const int64_t ntiles = (count + tile - 1) / tile, nchunks = (count + RK_CHUNK - 1) / RK_CHUNK;
  return 8 * count + ntiles * (256 * 4 + (int64_t)sizeof(RankTileSum) + (int64_t)sizeof(RankTileCarry) + 8 + (int64_t)sizeof(RankBest)) + 8 * nchunks +
         (int64_t)sizeof(RankTotals);
}

// refuses a count whose single-vector workspace exceeds the cap, before anything is allocated
Plan plan_for(const mvk_index* h, int Q, bool bank, int64_t count) {
  Plan p;
  p.tile = h->plan_tile_rows ? h->plan_tile_rows : 1024;
  p.ntiles = (int)((count + p.tile - 1) / p.tile);
  p.nchunks = (int)((count + RK_CHUNK - 1) / RK_CHUNK);
  const int64_t cap = h->plan_work_cap ? h->plan_work_cap : RK_WORK_CAP_BYTES;
  const int64_t per = vector_bytes(count, p.tile), fixed = bank ? 4 * count : 0;
  need(per + fixed <= cap, "the workspace of one vector over " + std::to_string(count) + " rows takes " + std::to_string(per + fixed) + " bytes: the cap is " +
                               std::to_string(cap) + "; rank fewer rows per call");
  int64_t fit = (cap - fixed) / per;  // one at the least, whole score tiles where there are several
  if (fit > RK_QT) fit = fit / RK_QT * RK_QT;
  if (h->plan_vector_group) fit = std::min<int64_t>(fit, h->plan_vector_group);
  p.group = (int)std::min<int64_t>(fit, Q);
  return p;
}

void grow_for(mvk_index* h, const Plan& pl, int64_t count, int slots, bool bank) {
  const size_t G = (size_t)pl.group, Qs = (G + RK_QT - 1) / RK_QT * RK_QT;
  grow(h->vT, h->vT_n, (size_t)h->P * Qs);
  grow(h->bv, h->bv_n, Qs);
  grow(h->keys_a, h->keys_a_n, G * count);
  grow(h->keys_b, h->keys_b_n, G * count);
  grow(h->hist, h->hist_n, G * pl.ntiles * 256);
  if (bank) grow(h->bank, h->bank_n, (size_t)count);
  grow(h->sums, h->sums_n, G * pl.ntiles);
  grow(h->carry, h->carry_n, G * pl.ntiles);
  grow(h->totals, h->totals_n, G);
  grow(h->p_u2, h->p_u2_n, G * pl.ntiles);
  grow(h->p_ap, h->p_ap_n, G * pl.nchunks);
  grow(h->p_best, h->p_best_n, G * pl.ntiles);
  grow(h->o_n, h->o_n_n, (size_t)slots * 3);
  grow(h->o_u2, h->o_u2_n, (size_t)slots);
  grow(h->o_ap, h->o_ap_n, (size_t)slots);
  grow(h->o_thres, h->o_thres_n, (size_t)slots);
  grow(h->o_best, h->o_best_n, (size_t)slots * 2);
}

// ---- the stages' clock: tick(stage) closes the interval since the last tick and charges it to `stage` (1 score, 2 sort, 3 statistics; 0 opens the call)

struct Clock {
  mvk_index* h;
  size_t used = 0;
  explicit Clock(mvk_index* h_) : h(h_) {
    h->timed = false;
    h->ev_stage.clear();
    tick(0);
  }
  void tick(int stage) {
    if (used == h->ev.size()) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreate(&e));
      h->ev.push_back(e);
    }
    HIPCHK(hipEventRecord(h->ev[used++], h->stream));
    h->ev_stage.push_back(stage);
  }
  void done() {  // the stream is idle
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = 1; i < used; ++i) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, h->ev[i - 1], h->ev[i]));
      ms[h->ev_stage[i]] += t;
    }
    ms[0] = ms[1] + ms[2] + ms[3];
    std::copy(ms, ms + 4, h->ms);
    h->timed = true;
  }
};

template <class Launch>
void by_tile(int tile, Launch launch) {
  switch (tile) {
    case 256: launch(std::integral_constant<int, 256>{}); break;
    case 512: launch(std::integral_constant<int, 512>{}); break;
    default: launch(std::integral_constant<int, 1024>{}); break;
  }
}

// the group's vectors [q0, q0 + nq) transposed and their bv, then keys_a [nq][count] of rows [first, first + count)
void score_group(mvk_index* h, int q0, int nq, int64_t first, int64_t count) {
  const int Qs = (nq + RK_QT - 1) / RK_QT * RK_QT;
  if (h->P == 512) hipLaunchKernelGGL(rank_vector_prep_kernel<512>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, h->vdev + (size_t)q0 * h->P, h->wd, h->vT, h->bv, nq, Qs);
  else hipLaunchKernelGGL(rank_vector_prep_kernel<768>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, h->vdev + (size_t)q0 * h->P, h->wd, h->vT, h->bv, nq, Qs);
  launched("rank_vector_prep_kernel");
  RankScoreArgs a{};
  a.first = first; a.count = count; a.nblocks = (count + RK_BR - 1) / RK_BR; a.nq = nq; a.Qs = Qs; a.same_idx = h->same_idx; a.cls = h->cls; a.keys = h->keys_a;
  const dim3 grid((unsigned)(Qs / RK_QT), (unsigned)std::min<int64_t>(a.nblocks, RK_GRID_Y), (unsigned)((a.nblocks + RK_GRID_Y - 1) / RK_GRID_Y));
  if (h->P == 512) hipLaunchKernelGGL(rank_score_kernel<512>, grid, dim3(RK_BR), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a);
  else hipLaunchKernelGGL(rank_score_kernel<768>, grid, dim3(RK_BR), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a);
  launched("rank_score_kernel");
}

void fold_group(mvk_index* h, int nq, int64_t count, bool first_group) {
  hipLaunchKernelGGL(rank_bank_fold_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, h->keys_a, h->bank, (long long)count, nq, first_group ? 1 : 0);
  launched("rank_bank_fold_kernel");
}

// four passes of eight bits over nq arrays of `count` keys: a -> b -> a -> b -> a.  The sorted keys are in `a` again
void sort_keys(mvk_index* h, const Plan& pl, uint32_t* a, uint32_t* b, int nq, int64_t count) {
  const dim3 grid((unsigned)pl.ntiles, (unsigned)nq);
  for (int pass = 0; pass < 4; ++pass) {
    const uint32_t* in = pass % 2 ? b : a;
    uint32_t* out = pass % 2 ? a : b;
    by_tile(pl.tile, [&](auto tr) {
      constexpr int TR = decltype(tr)::value;
      hipLaunchKernelGGL(rank_hist_kernel<TR>, grid, dim3(TR), 0, h->stream, in, h->hist, (int)count, 8 * pass);
      launched("rank_hist_kernel");
      hipLaunchKernelGGL(rank_digit_scan_kernel, dim3((unsigned)nq), dim3(256 * RK_SCAN_SEGS), 0, h->stream, h->hist, pl.ntiles);
      launched("rank_digit_scan_kernel");
      hipLaunchKernelGGL(rank_scatter_kernel<TR>, grid, dim3(TR), 0, h->stream, in, out, h->hist, (int)count, 8 * pass);
      launched("rank_scatter_kernel");
    });
  }
}

// the prefixes of nq sorted key arrays: sums, carry, totals
void scan_keys(mvk_index* h, const Plan& pl, const uint32_t* keys, int nq, int64_t count) {
  const dim3 grid((unsigned)pl.ntiles, (unsigned)nq);
  by_tile(pl.tile, [&](auto tr) {
    constexpr int TR = decltype(tr)::value;
    hipLaunchKernelGGL(rank_tile_sums_kernel<TR>, grid, dim3(TR), 0, h->stream, keys, h->sums, (int)count);
    launched("rank_tile_sums_kernel");
    hipLaunchKernelGGL(rank_tile_scan_kernel<TR>, dim3((unsigned)nq), dim3(256), 0, h->stream, h->sums, h->carry, h->totals, pl.ntiles);
    launched("rank_tile_scan_kernel");
  });
}

RankStatsArgs stats_args(mvk_index* h, const Plan& pl, const uint32_t* keys, int64_t count) {
  RankStatsArgs a{};
  a.keys = keys; a.carry = h->carry; a.totals = h->totals; a.u2 = h->p_u2; a.ap = h->p_ap; a.best = h->p_best; a.count = (int)count; a.nchunks = pl.nchunks;
  return a;
}

// the statistics of nq sorted key arrays -> result slots slot0 ..
void stats_keys(mvk_index* h, const Plan& pl, const uint32_t* keys, int nq, int64_t count, int slot0) {
  scan_keys(h, pl, keys, nq, count);
  const RankStatsArgs a = stats_args(h, pl, keys, count);
  by_tile(pl.tile, [&](auto tr) {
    constexpr int TR = decltype(tr)::value;
    hipLaunchKernelGGL((rank_stats_kernel<TR, false>), dim3((unsigned)pl.ntiles, (unsigned)nq), dim3(TR), 0, h->stream, a);
  });
  launched("rank_stats_kernel");
  const RankOut out{h->o_n, h->o_u2, h->o_ap, h->o_thres, h->o_best};
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream, h->totals, h->p_u2, h->p_ap, h->p_best, pl.ntiles, pl.nchunks, (int)count, slot0, out);
  launched("rank_finish_kernel");
}

void upload_vectors(mvk_index* h, const float* v, int Q) {
  grow(h->vdev, h->vdev_n, (size_t)Q * h->P);
  HIPCHK(hipMemcpyAsync(h->vdev, v, (size_t)Q * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
}

}  // namespace

extern "C" {

const char* mvk_last_error(mvk_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvk_create(int device, int proj_dim, const float* Wm, int same_idx, mvk_index** out) try {
  need(out != nullptr, "out is NULL");
  *out = nullptr;
  need(proj_dim == 512 || proj_dim == 768, "proj_dim = " + std::to_string(proj_dim) + ": the matcher runs on 512 or 768 features");
  need(same_idx == 0 || same_idx == 1, "same_idx = " + std::to_string(same_idx) + ": 0 or 1");
  need(Wm != nullptr, "the matcher weight is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw std::runtime_error("no HIP device: the ranking index has no CPU fallback");
  need(device >= 0 && device < ndev, "device " + std::to_string(device) + " of " + std::to_string(ndev));
  HIPCHK(hipSetDevice(device));
  mvk_index* h = new mvk_index();
  h->device = device; h->P = proj_dim; h->same_idx = same_idx;
  try {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    float* wm = nullptr;
    HIPCHK(hipMalloc((void**)&h->wd, (size_t)3 * h->P * sizeof(float)));
    HIPCHK(hipMalloc((void**)&wm, (size_t)6 * h->P * sizeof(float)));
    hipError_t e = hipMemcpyAsync(wm, Wm, (size_t)6 * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(rank_weight_delta_kernel, dim3((3 * h->P + 255) / 256), dim3(256), 0, h->stream, wm, h->wd, h->P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(wm);
    hipchk(e, "uploading the matcher weight");
  } catch (...) {
    mvk_destroy(h);
    throw;
  }
  *out = h;
  return MVK_OK;
} catch (...) { return on_exception(nullptr); }

void mvk_destroy(mvk_index* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->cls, (void*)h->wd, (void*)h->vdev, (void*)h->vT, (void*)h->bv, (void*)h->keys_a, (void*)h->keys_b, (void*)h->hist,
                  (void*)h->bank, (void*)h->sums, (void*)h->carry, (void*)h->totals, (void*)h->p_u2, (void*)h->p_ap, (void*)h->p_best, (void*)h->o_n, (void*)h->o_u2,
                  (void*)h->o_best, (void*)h->o_ap, (void*)h->o_thres, (void*)h->c_thres, (void*)h->c_tp, (void*)h->c_fp})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int mvk_add(mvk_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  need(n >= 0, "n = " + std::to_string(n) + " rows");
  need(n <= MVK_MAX_ROWS - h->n, "the index would hold more than 2^31 - 2 rows");
  if (n == 0) return MVK_OK;
  need(embed != nullptr, "the embeddings are NULL");
  HIPCHK(hipSetDevice(h->device));
  reserve_rows(h, h->n + n);
  HIPCHK(hipMemcpyAsync(h->U + (size_t)h->n * h->P, embed, (size_t)n * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->cls + h->n, 0, (size_t)n, h->stream));
  if (h->P == 512) hipLaunchKernelGGL(rank_row_term_kernel<512>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  else hipLaunchKernelGGL(rank_row_term_kernel<768>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  launched("rank_row_term_kernel");
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's buffer is free again, and the rows count only once they are there)
  h->n += n;
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_reset(mvk_index* h) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  h->n = 0;
  return MVK_OK;
} catch (...) { return on_exception(h); }

int64_t mvk_count(mvk_index* h) { return h ? h->n : 0; }

int mvk_set_classes(mvk_index* h, const uint8_t* cls, int64_t first, int64_t n) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  need(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  if (n == 0) return MVK_OK;
  need(cls != nullptr, "the classes are NULL");
  for (int64_t i = 0; i < n; ++i) need(cls[i] <= 1, "cls[" + std::to_string(i) + "] = " + std::to_string((int)cls[i]) + ": a class is 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->cls + first, cls, (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_rank(mvk_index* h, const float* v, int Q, int bank, int64_t first, int64_t count, int64_t* n, int64_t* u2, double* ap, float* best_thres, int64_t* best) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  h->timed = false;
  check_range(h, v, Q, first, count);
  need(n != nullptr && u2 != nullptr && ap != nullptr && best_thres != nullptr && best != nullptr, "an output buffer is NULL");
  const int S = Q + (bank ? 1 : 0);
  if (count == 0) {  // nothing to rank
    std::fill(n, n + 3 * (size_t)S, (int64_t)0);
    std::fill(u2, u2 + S, (int64_t)0);
    std::fill(ap, ap + S, std::numeric_limits<double>::quiet_NaN());
    std::fill(best_thres, best_thres + S, std::numeric_limits<float>::quiet_NaN());
    std::fill(best, best + 2 * (size_t)S, (int64_t)0);
    return MVK_OK;
  }
  const Plan pl = plan_for(h, Q, bank != 0, count);
  HIPCHK(hipSetDevice(h->device));
  grow_for(h, pl, count, S, bank != 0);
  upload_vectors(h, v, Q);
  Clock clock(h);
  for (int q0 = 0; q0 < Q; q0 += pl.group) {
    const int nq = std::min(pl.group, Q - q0);
    score_group(h, q0, nq, first, count);
    if (bank) fold_group(h, nq, count, q0 == 0);
    clock.tick(1);
    sort_keys(h, pl, h->keys_a, h->keys_b, nq, count);
    clock.tick(2);
    stats_keys(h, pl, h->keys_a, nq, count, q0);
    clock.tick(3);
  }
  if (bank) {
    sort_keys(h, pl, h->bank, h->keys_b, 1, count);
    clock.tick(2);
    stats_keys(h, pl, h->bank, 1, count, Q);
    clock.tick(3);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  clock.done();
  static_assert(sizeof(long long) == sizeof(int64_t), "the integers are copied as they are");
  // (every copy lands or none is reported: they go to buffers of the library's own first)
  std::vector<int64_t> hn((size_t)S * 3), hu((size_t)S), hb((size_t)S * 2);
  std::vector<double> ha((size_t)S);
  std::vector<float> ht((size_t)S);
  HIPCHK(hipMemcpy(hn.data(), h->o_n, hn.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hu.data(), h->o_u2, hu.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hb.data(), h->o_best, hb.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ha.data(), h->o_ap, ha.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ht.data(), h->o_thres, ht.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::copy(hn.begin(), hn.end(), n);
  std::copy(hu.begin(), hu.end(), u2);
  std::copy(hb.begin(), hb.end(), best);
  std::copy(ha.begin(), ha.end(), ap);
  std::copy(ht.begin(), ht.end(), best_thres);
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_curve(mvk_index* h, const float* v, int Q, int bank, int64_t first, int64_t count, int64_t* points) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  h->timed = false;
  check_range(h, v, Q, first, count);
  need(bank || Q == 1, "Q = " + std::to_string(Q) + " without the bank score: a curve is that of ONE ranking");
  need(points != nullptr, "points is NULL");
  if (count == 0) {  // an empty curve is held
    *points = 0;
    h->held = true;
    return MVK_OK;
  }
  const Plan pl = plan_for(h, Q, bank != 0, count);
  HIPCHK(hipSetDevice(h->device));
  grow_for(h, pl, count, 1, bank != 0);
  upload_vectors(h, v, Q);
  Clock clock(h);
  for (int q0 = 0; q0 < Q; q0 += pl.group) {
    const int nq = std::min(pl.group, Q - q0);
    score_group(h, q0, nq, first, count);
    if (bank) fold_group(h, nq, count, q0 == 0);
  }
  clock.tick(1);
  uint32_t* keys = bank ? h->bank : h->keys_a;
  sort_keys(h, pl, keys, h->keys_b, 1, count);
  clock.tick(2);
  scan_keys(h, pl, keys, 1, count);
  RankTotals tt{};
  HIPCHK(hipMemcpyAsync(&tt, h->totals, sizeof(tt), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (tt.groups < 0 || tt.groups > count) throw std::runtime_error("the curve reported " + std::to_string(tt.groups) + " tie groups");
  if (tt.groups > 0) {
    grow(h->c_thres, h->c_thres_n, (size_t)tt.groups);
    grow(h->c_tp, h->c_tp_n, (size_t)tt.groups);
    grow(h->c_fp, h->c_fp_n, (size_t)tt.groups);
    RankStatsArgs a = stats_args(h, pl, keys, count);
    a.c_thres = h->c_thres; a.c_tp = h->c_tp; a.c_fp = h->c_fp;
    by_tile(pl.tile, [&](auto tr) {
      constexpr int TR = decltype(tr)::value;
      hipLaunchKernelGGL((rank_stats_kernel<TR, true>), dim3((unsigned)pl.ntiles, 1u), dim3(TR), 0, h->stream, a);
    });
    launched("rank_stats_kernel");
  }
  clock.tick(3);
  HIPCHK(hipStreamSynchronize(h->stream));
  clock.done();
  *points = tt.groups;
  h->points = tt.groups;
  h->held = true;
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_fetch(mvk_index* h, float* thres, int64_t* tp, int64_t* fp) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  if (!h->held) throw StateError("no curve is held: mvk_fetch follows a successful mvk_curve, with no other call on the index in between");
  if (h->points == 0) return MVK_OK;
  need(thres != nullptr && tp != nullptr && fp != nullptr, "an output buffer is NULL");
  HIPCHK(hipSetDevice(h->device));
  // (every copy lands or none is reported: they go to buffers of the library's own first)
  std::vector<float> t((size_t)h->points);
  std::vector<int64_t> a((size_t)h->points), b((size_t)h->points);
  HIPCHK(hipMemcpy(t.data(), h->c_thres, t.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(a.data(), h->c_tp, a.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(b.data(), h->c_fp, b.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::copy(t.begin(), t.end(), thres);
  std::copy(a.begin(), a.end(), tp);
  std::copy(b.begin(), b.end(), fp);
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_kernel_ms(mvk_index* h, float* ms) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  need(ms != nullptr, "ms is NULL");
  need(h->timed, "the last call launched no kernel");
  std::copy(h->ms, h->ms + 4, ms);
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_test_plan(mvk_index* h, int tile_rows, int vector_group, int64_t work_cap_bytes) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  need(tile_rows == 0 || tile_rows == 256 || tile_rows == 512 || tile_rows == 1024, "tile_rows = " + std::to_string(tile_rows) + ": 0, 256, 512 or 1024");
  need(vector_group >= 0 && vector_group <= MVK_MAX_VECTORS, "vector_group = " + std::to_string(vector_group) + ": 0 .. 4096");
  need(work_cap_bytes >= 0, "work_cap_bytes = " + std::to_string(work_cap_bytes));
  h->plan_tile_rows = tile_rows; h->plan_vector_group = vector_group; h->plan_work_cap = work_cap_bytes;
  return MVK_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
