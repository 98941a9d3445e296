// libmemvul_bank.so: the anchor-bank audit over a kept corpus (include/memvul_bank.h; kernels and plan: bank_cover.h).  A library of its own, which no other
// library of this tree links against: their kernel sets, their source fingerprints and their lists of entries all stay as they are.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/memvul_bank.h"
#include "bank_cover.h"
#include "kept_index.h"

KEPT_ASSERT_ABI(MVB, MVB_MAX_VECTORS);
static_assert(MVB_ERR_STATE == KEPT_ERR_STATE, "the public header and kept_index.h disagree");

namespace {
const KeptKernels kBankKernels = {bank_weight_delta_kernel, {bank_row_term_kernel<512>, bank_row_term_kernel<768>}, {bank_vector_prep_kernel<512>, bank_vector_prep_kernel<768>}};
}

struct mvb_index : KeptIndex {
  mvb_index() : KeptIndex(&kBankKernels, true, 2) {}
  // workspace (grows, never shrinks)
  float* thr = nullptr;               // the thresholds [Q]
  size_t thr_n = 0;
  unsigned long long* out = nullptr;  // the integers of a reading call
  size_t out_n = 0;
  uint16_t* mult = nullptr;           // [count]
  int32_t* sole_of = nullptr;         // [count]
  size_t mult_n = 0, sole_of_n = 0;
  int* tiles = nullptr;               // overlap: the tile pairs of the upper triangle
  size_t tiles_n = 0;
  uint8_t* taken = nullptr;           // greedy: [Q]
  long long* part = nullptr;          // greedy: [Q][chunks][2]
  int32_t* order = nullptr;           // greedy: [Q]
  long long* gained = nullptr;        // greedy: [Q][2]
  BankGreedyState* gstate = nullptr;
  size_t taken_n = 0, part_n = 0, order_n = 0, gained_n = 0;
  // the held marking
  bool held = false;
  int Q = 0;
  int64_t first = 0, count = 0, W = 0;
  unsigned long long *bits = nullptr, *pos = nullptr, *covered = nullptr;  // B [Q][W]; class words [W]; covered rows [W]
  size_t bits_n = 0, pos_n = 0, covered_n = 0;
  int plan_block_rows = 0, plan_vector_group = 0, plan_word_chunk = 0;  // mvb_test_plan; 0 = the library's own choice
};

namespace {

template <int P>
void launch_mark(mvb_index* h, int block_rows, dim3 grid, const BankMarkArgs& a) {
  by_block_rows(block_rows, [&](auto br) {
    constexpr int BR = decltype(br)::value;
    hipLaunchKernelGGL((bank_mark_kernel<P, BR>), grid, dim3(BR), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a);
  });
  launched("bank_mark_kernel");
}

void drop_marking(mvb_index* h) {
  h->held = false;
  h->Q = 0;
  h->first = h->count = h->W = 0;
}

void need_marking(const mvb_index* h, const char* who) {
  if (!h->held) throw StateError(std::string("no marking is held: ") + who + " follows a successful mvb_mark, with no call that drops the marking in between");
}

// words per workgroup of a reading kernel: the test plan's, or `own`; never so many that a workgroup's 32-bit counters could overflow
int word_chunk(const mvb_index* h, int64_t own) {
  const int64_t c = h->plan_word_chunk ? h->plan_word_chunk : own;
  return (int)std::max<int64_t>(1, std::min<int64_t>(c, 1 << 24));
}

struct Timed {  // the events around a call's launches
  mvb_index* h;
  explicit Timed(mvb_index* h_) : h(h_) {
    h->timed = 0;
    HIPCHK(hipEventRecord(h->ev[0], h->stream));
  }
  void done() {
    HIPCHK(hipEventRecord(h->ev[1], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timed = 1;
  }
};

}  // namespace

extern "C" {

const char* mvb_last_error(mvb_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvb_create(int device, int proj_dim, const float* Wm, int same_idx, mvb_index** out) try {
  kept_create("bank audit", mvb_destroy, device, proj_dim, Wm, same_idx, out, [](mvb_index* h) { HIPCHK(hipMalloc((void**)&h->gstate, sizeof(BankGreedyState))); });
  return MVB_OK;
} catch (...) { return on_exception(nullptr); }

void mvb_destroy(mvb_index* h) {
  if (!h) return;
  kept_destroy_common(h, {h->thr, h->out, h->mult, h->sole_of, h->tiles, h->taken, h->part, h->order, h->gained, h->gstate, h->bits, h->pos, h->covered});
  delete h;
}

int mvb_add(mvb_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  kept_add(h, embed, n);
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_reset(mvb_index* h) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  h->n = 0;
  return MVB_OK;
} catch (...) { return on_exception(h); }

int64_t mvb_count(mvb_index* h) { return h ? h->n : 0; }

int mvb_set_classes(mvb_index* h, const uint8_t* cls, int64_t first, int64_t n) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  kept_set_classes(h, cls, first, n);
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_mark(mvb_index* h, const float* v, int Q, const float* thres, int64_t first, int64_t count) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  h->timed = 0;
  check_range(h, "vectors", v, Q, first, count);
  check_thresholds(thres, Q);
  const int64_t W = (count + 63) / 64;
  const int64_t bytes = 8 * (int64_t)Q * W;
  need(bytes <= MVB_MAX_MARK_BYTES, "the marking of " + std::to_string(Q) + " vectors over " + std::to_string(count) + " rows takes " + std::to_string(bytes) +
                                        " bytes: at most " + std::to_string((long long)MVB_MAX_MARK_BYTES) + " (MVB_MAX_MARK_BYTES) are held; mark fewer vectors or rows");
  if (count == 0) {  // nothing to claim: an empty marking is held
    h->held = true;
    h->Q = Q; h->first = first; h->count = 0; h->W = 0;
    return MVB_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const int block_rows = h->plan_block_rows ? h->plan_block_rows : 256;
  const int64_t nblocks = (count + block_rows - 1) / block_rows;
  const int group = std::min(h->plan_vector_group ? h->plan_vector_group : Q, Q);  // (vT of 4096 vectors is 8 MB at 512 features: one group unless the test plan says otherwise)
  const int Qs_max = (group + BK_QT - 1) / BK_QT * BK_QT;
  grow(h->thr, h->thr_n, (size_t)Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs_max);
  grow(h->bv, h->bv_n, (size_t)Qs_max);
  grow(h->bits, h->bits_n, (size_t)Q * W);
  grow(h->pos, h->pos_n, (size_t)W);
  grow(h->covered, h->covered_n, (size_t)W);
  kept_upload_vectors(h, v, Q);
  HIPCHK(hipMemcpyAsync(h->thr, thres, (size_t)Q * sizeof(float), hipMemcpyHostToDevice, h->stream));
  Timed t(h);
  for (int q0 = 0; q0 < Q; q0 += group) {
    const int nq = std::min(group, Q - q0);
    const int Qs = (nq + BK_QT - 1) / BK_QT * BK_QT;
    kept_vector_prep(h, q0, nq, Qs);
    BankMarkArgs a{};
    a.first = first; a.count = count; a.nblocks = nblocks; a.W = W; a.nq = nq; a.Qs = Qs; a.q0 = q0; a.same_idx = h->same_idx; a.thr = h->thr;
    a.bits = h->bits + (size_t)q0 * W;  // the group's slice of the full matrix
    const dim3 grid((unsigned)(Qs / BK_QT), (unsigned)std::min<int64_t>(nblocks, BK_GRID_Y), (unsigned)((nblocks + BK_GRID_Y - 1) / BK_GRID_Y));
    if (h->P == 512) launch_mark<512>(h, block_rows, grid, a);
    else launch_mark<768>(h, block_rows, grid, a);
  }
  hipLaunchKernelGGL(bank_class_words_kernel, dim3((unsigned)((W + 3) / 4)), dim3(256), 0, h->stream, h->cls, h->pos, (long long)first, (long long)count, (long long)W);
  launched("bank_class_words_kernel");
  t.done();
  h->held = true;
  h->Q = Q; h->first = first; h->count = count; h->W = W;
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_totals(mvb_index* h, int64_t* claimed) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  need_marking(h, "mvb_totals");
  need(claimed != nullptr, "the output buffer is NULL");
  const size_t n = (size_t)h->Q * 2;
  if (h->count == 0) {
    h->timed = 0;
    std::fill(claimed, claimed + n, (int64_t)0);
    return MVB_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  grow(h->out, h->out_n, n);
  Timed t(h);
  hipLaunchKernelGGL(bank_totals_kernel, dim3((unsigned)h->Q), dim3(256), 0, h->stream, h->bits, h->pos, (long long*)h->out, (long long)h->W);
  launched("bank_totals_kernel");
  t.done();
  static_assert(sizeof(long long) == sizeof(int64_t), "the integers are copied as they are");
  HIPCHK(hipMemcpy(claimed, h->out, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_multiplicity(mvb_index* h, int64_t* hist, int64_t* sole, uint16_t* mult, int32_t* sole_of) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  need_marking(h, "mvb_multiplicity");
  need(hist != nullptr && sole != nullptr, "an output buffer is NULL");
  const size_t nh = (size_t)2 * (h->Q + 1), ns = (size_t)2 * h->Q;
  if (h->count == 0) {
    h->timed = 0;
    std::fill(hist, hist + nh, (int64_t)0);
    std::fill(sole, sole + ns, (int64_t)0);
    return MVB_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  grow(h->out, h->out_n, nh + ns);
  if (mult) grow(h->mult, h->mult_n, (size_t)h->count);
  if (sole_of) grow(h->sole_of, h->sole_of_n, (size_t)h->count);
  const int chunk = word_chunk(h, 16);  // 16 words = one 128-byte line of every row of B
  Timed t(h);
  HIPCHK(hipMemsetAsync(h->out, 0, (nh + ns) * sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(bank_multiplicity_kernel, dim3((unsigned)((h->W + chunk - 1) / chunk)), dim3(256), 0, h->stream, h->bits, h->pos, h->Q, (long long)h->W,
                     (long long)h->count, chunk, h->out, h->out + nh, mult ? h->mult : nullptr, sole_of ? h->sole_of : nullptr);
  launched("bank_multiplicity_kernel");
  t.done();
  // (every copy lands or none is reported: they go to buffers of the library's own first)
  std::vector<int64_t> small(nh + ns);
  std::vector<uint16_t> m(mult ? (size_t)h->count : 0);
  std::vector<int32_t> so(sole_of ? (size_t)h->count : 0);
  HIPCHK(hipMemcpy(small.data(), h->out, (nh + ns) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (mult) HIPCHK(hipMemcpy(m.data(), h->mult, m.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
  if (sole_of) HIPCHK(hipMemcpy(so.data(), h->sole_of, so.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::copy(small.begin(), small.begin() + nh, hist);
  std::copy(small.begin() + nh, small.end(), sole);
  if (mult) std::copy(m.begin(), m.end(), mult);
  if (sole_of) std::copy(so.begin(), so.end(), sole_of);
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_overlap(mvb_index* h, int64_t* overlap) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  need_marking(h, "mvb_overlap");
  need(overlap != nullptr, "the output buffer is NULL");
  const int Q = h->Q;
  const size_t n = (size_t)Q * Q * 2;
  if (h->count == 0) {
    h->timed = 0;
    std::fill(overlap, overlap + n, (int64_t)0);
    return MVB_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const int nt = (Q + BK_OT - 1) / BK_OT;
  std::vector<int> tiles;
  for (int a = 0; a < nt; ++a)
    for (int b = a; b < nt; ++b) {  // the upper triangle of tiles
      tiles.push_back(a);
      tiles.push_back(b);
    }
  grow(h->out, h->out_n, n);
  grow(h->tiles, h->tiles_n, tiles.size());
  // words per workgroup: at most 16 chunks per tile pair (every chunk ends in up to 2 048 atomics), whole staging steps
  const int chunk = word_chunk(h, std::max<int64_t>(BK_OW, ((h->W + 15) / 16 + BK_OW - 1) / BK_OW * BK_OW));
  const int64_t nchunks = (h->W + chunk - 1) / chunk;
  need(nchunks <= 65535, "the overlap grid would have " + std::to_string(nchunks) + " word chunks");
  HIPCHK(hipMemcpyAsync(h->tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  Timed t(h);
  HIPCHK(hipMemsetAsync(h->out, 0, n * sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(bank_overlap_kernel, dim3((unsigned)(tiles.size() / 2), (unsigned)nchunks), dim3(256), 0, h->stream, h->bits, h->pos, Q, (long long)h->W, chunk,
                     h->tiles, h->out);
  launched("bank_overlap_kernel");
  hipLaunchKernelGGL(bank_mirror_kernel, dim3((unsigned)(((size_t)Q * Q + 255) / 256)), dim3(256), 0, h->stream, h->out, Q);
  launched("bank_mirror_kernel");
  t.done();  // (the pageable tile upload above is done with `tiles` by now as well)
  HIPCHK(hipMemcpy(overlap, h->out, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_greedy(mvb_index* h, int64_t w_pos, int64_t w_neg, const uint8_t* fixed, int max_rounds, int* rounds, int32_t* order, int64_t* gained) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  need_marking(h, "mvb_greedy");
  need(w_pos >= 0 && w_pos <= MVB_MAX_WEIGHT, "w_pos = " + std::to_string(w_pos) + ": 0 <= w <= 2^20");
  need(w_neg >= 0 && w_neg <= MVB_MAX_WEIGHT, "w_neg = " + std::to_string(w_neg) + ": 0 <= w <= 2^20");
  need(max_rounds >= 0, "max_rounds = " + std::to_string(max_rounds));
  need(rounds != nullptr, "rounds is NULL");
  const int Q = h->Q;
  int free_vectors = 0;
  for (int q = 0; q < Q; ++q) free_vectors += !(fixed && fixed[q]);
  const int limit = std::min(max_rounds, free_vectors);
  need(limit == 0 || (order != nullptr && gained != nullptr), "an output buffer is NULL");
  if (h->count == 0 || limit == 0 || w_pos == 0) {  // (no gain can be positive)
    h->timed = 0;
    *rounds = 0;
    return MVB_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  const int chunk = word_chunk(h, 1024);
  const int64_t nchunks = (h->W + chunk - 1) / chunk;
  need(nchunks <= 65535, "the gain grid would have " + std::to_string(nchunks) + " word chunks");
  grow(h->taken, h->taken_n, (size_t)Q);
  grow(h->part, h->part_n, (size_t)Q * nchunks * 2);
  grow(h->order, h->order_n, (size_t)Q);
  grow(h->gained, h->gained_n, (size_t)Q * 2);
  std::vector<uint8_t> taken((size_t)Q, 0);
  for (int q = 0; q < Q; ++q) taken[q] = fixed && fixed[q] ? 1 : 0;
  HIPCHK(hipMemcpyAsync(h->taken, taken.data(), (size_t)Q, hipMemcpyHostToDevice, h->stream));
  Timed t(h);
  hipLaunchKernelGGL(bank_cover_init_kernel, dim3((unsigned)((h->W + 255) / 256)), dim3(256), 0, h->stream, h->bits, h->taken, Q, (long long)h->W, h->covered, h->gstate);
  launched("bank_cover_init_kernel");
  BankGreedyState st{0, 0};
  for (int r = 0; r < limit && !st.done;) {
    const int upto = std::min(limit, r + 8);  // the host looks at the stop condition every eight rounds; launches after `done` do nothing
    for (; r < upto; ++r) {
      hipLaunchKernelGGL(bank_gain_kernel, dim3((unsigned)Q, (unsigned)nchunks), dim3(256), 0, h->stream, h->bits, h->pos, h->covered, h->taken, (long long)h->W, chunk,
                         (int)nchunks, h->gstate, h->part);
      launched("bank_gain_kernel");
      hipLaunchKernelGGL(bank_pick_kernel, dim3(1), dim3(BK_PICK_THREADS), 0, h->stream, h->bits, h->covered, h->taken, Q, (long long)h->W, (int)nchunks, h->part,
                         (long long)w_pos, (long long)w_neg, limit, h->gstate, h->order, h->gained);
      launched("bank_pick_kernel");
    }
    HIPCHK(hipMemcpyAsync(&st, h->gstate, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  t.done();
  if (st.rounds < 0 || st.rounds > limit) throw std::runtime_error("the greedy cover reported " + std::to_string(st.rounds) + " rounds");
  std::vector<int32_t> o((size_t)st.rounds);
  std::vector<int64_t> g((size_t)st.rounds * 2);
  if (st.rounds) {
    HIPCHK(hipMemcpy(o.data(), h->order, o.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g.data(), h->gained, g.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  std::copy(o.begin(), o.end(), order);
  std::copy(g.begin(), g.end(), gained);
  *rounds = st.rounds;
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_kernel_ms(mvb_index* h, float* ms) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  kept_kernel_ms(h, ms, "the last call launched no kernel");
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_test_plan(mvb_index* h, int block_rows, int vector_group, int word_chunk) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  check_block_rows(block_rows);
  need(vector_group >= 0 && vector_group <= MVB_MAX_VECTORS, "vector_group = " + std::to_string(vector_group) + ": 0 .. 4096");
  need(word_chunk >= 0 && word_chunk <= (1 << 24), "word_chunk = " + std::to_string(word_chunk) + ": 0 .. 2^24");
  h->plan_block_rows = block_rows; h->plan_vector_group = vector_group; h->plan_word_chunk = word_chunk;
  return MVB_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
