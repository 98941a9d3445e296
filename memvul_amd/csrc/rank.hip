// libmemvul_rank.so: per-anchor ranking quality over a kept corpus (include/memvul_rank.h; kernels and plan: rank_sort.h).  A library of its own, which no other
// library of this tree links against: their kernel sets, their source fingerprints and their lists of entries all stay as they are.  The index over the kept
// corpus is kept_index.h's; what stands here is the library's own: the plan, the sort and the statistics, the stages' clock and the held curve.
#include <hip/hip_runtime.h>

#include <cstring>
#include <limits>
#include <vector>

#include "../../include/memvul_rank.h"
#include "rank_sort.h"
#include "kept_index.h"

KEPT_ASSERT_ABI(MVK, MVK_MAX_VECTORS);
static_assert(MVK_ERR_STATE == KEPT_ERR_STATE, "the public header and kept_index.h disagree");

namespace {
const KeptKernels kRankKernels = {rank_weight_delta_kernel, {rank_row_term_kernel<512>, rank_row_term_kernel<768>}, {rank_vector_prep_kernel<512>, rank_vector_prep_kernel<768>}};
}

struct mvk_index : KeptIndex {
  mvk_index() : KeptIndex(&kRankKernels, true, 0) {}  // (no event of the base: the stages' clock below keeps its own, and `timed` is 0 or 1)
  std::vector<hipEvent_t> ev_clock;   // the stage boundaries of a call, in order; created as needed, kept
  std::vector<int> ev_stage;          // the stage that ends at each event of the last call (-1: none)
  float ms[4] = {0.f, 0.f, 0.f, 0.f}; // the last call: whole, score, sort, statistics
  // workspace (grows, never shrinks)
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
};

namespace {

void drop_curve(mvk_index* h) {
  h->held = false;
  h->points = 0;
}

void check_rank_range(const mvk_index* h, const float* v, int Q, int64_t first, int64_t count) {
  check_range(h, "vectors", v, Q, first, count);
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
    h->timed = 0;
    h->ev_stage.clear();
    tick(0);
  }
  void tick(int stage) {
    if (used == h->ev_clock.size()) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreate(&e));
      h->ev_clock.push_back(e);
    }
    HIPCHK(hipEventRecord(h->ev_clock[used++], h->stream));
    h->ev_stage.push_back(stage);
  }
  void done() {  // the stream is idle
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = 1; i < used; ++i) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, h->ev_clock[i - 1], h->ev_clock[i]));
      ms[h->ev_stage[i]] += t;
    }
    ms[0] = ms[1] + ms[2] + ms[3];
    std::copy(ms, ms + 4, h->ms);
    h->timed = 1;
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
  kept_vector_prep(h, q0, nq, Qs);
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

}  // namespace

extern "C" {

const char* mvk_last_error(mvk_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvk_create(int device, int proj_dim, const float* Wm, int same_idx, mvk_index** out) try {
  kept_create("ranking index", mvk_destroy, device, proj_dim, Wm, same_idx, out);
  return MVK_OK;
} catch (...) { return on_exception(nullptr); }

void mvk_destroy(mvk_index* h) {
  if (!h) return;
  kept_destroy_common(h, {h->keys_a, h->keys_b, h->hist, h->bank, h->sums, h->carry, h->totals, h->p_u2, h->p_ap, h->p_best, h->o_n, h->o_u2, h->o_best, h->o_ap, h->o_thres,
                          h->c_thres, h->c_tp, h->c_fp});
  for (hipEvent_t e : h->ev_clock)  // (the stream they were recorded on is drained and gone)
    if (e) (void)hipEventDestroy(e);
  delete h;
}

int mvk_add(mvk_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  kept_add(h, embed, n);
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
  kept_set_classes(h, cls, first, n);
  return MVK_OK;
} catch (...) { return on_exception(h); }

int mvk_rank(mvk_index* h, const float* v, int Q, int bank, int64_t first, int64_t count, int64_t* n, int64_t* u2, double* ap, float* best_thres, int64_t* best) try {
  if (!h) return fail(nullptr, MVK_ERR_ARG, "index is NULL");
  drop_curve(h);
  h->timed = 0;
  check_rank_range(h, v, Q, first, count);
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
  kept_upload_vectors(h, v, Q);
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
  h->timed = 0;
  check_rank_range(h, v, Q, first, count);
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
  kept_upload_vectors(h, v, Q);
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
  need(h->timed > 0, "the last call launched no kernel");
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
