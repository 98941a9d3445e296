// libmemvul_bank.so: the anchor-bank audit over a kept corpus (include/memvul_bank.h; kernels and plan: bank_cover.h).  A library of its own, which no other
// library of this tree links against: their kernel sets, their source fingerprints and their lists of entries all stay as they are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/memvul_bank.h"
#include "bank_cover.h"

struct mvb_index {
  int device = 0, P = 0, same_idx = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};  // bracket the launches of a call
  bool timed = false;
  float *U = nullptr, *sa = nullptr;  // rows [cap][P], row terms [cap]
  uint8_t* cls = nullptr;             // [cap]
  int64_t n = 0, cap = 0;
  float* wd = nullptr;                // [3][P] class-difference weights
  // workspace (grows, never shrinks)
  float *vdev = nullptr, *vT = nullptr, *bv = nullptr, *thr = nullptr;  // the vectors [Q][P]; one group transposed [P][Qs]; its bv [Qs]; the thresholds [Q]
  size_t vdev_n = 0, vT_n = 0, bv_n = 0, thr_n = 0;
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
  std::string err;
};

namespace {

thread_local std::string g_err;  // errors with no index to hang them on (mvb_create)

struct Refusal : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct StateError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(mvb_index* h, int code, const std::string& msg) {
  (h ? h->err : g_err) = msg;
  return code;
}

int on_exception(mvb_index* h) noexcept {
  try {
    try {
      throw;
    } catch (const Refusal& e) {
      return fail(h, MVB_ERR_ARG, e.what());
    } catch (const StateError& e) {
      return fail(h, MVB_ERR_STATE, e.what());
    } catch (const std::bad_alloc&) {
      return fail(h, MVB_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
      return fail(h, MVB_ERR_HIP, e.what());
    } catch (...) {
      return fail(h, MVB_ERR_INTERNAL, "unknown C++ exception");
    }
  } catch (...) {  // (the message itself could not be stored)
    return MVB_ERR_INTERNAL;
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

void reserve_rows(mvb_index* h, int64_t want) {
  if (want <= h->cap) return;
  const int64_t cap = std::max<int64_t>(want, std::min<int64_t>(h->cap + h->cap / 2, MVB_MAX_ROWS));
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

template <int P>
void launch_mark(mvb_index* h, int block_rows, dim3 grid, const BankMarkArgs& a) {
  switch (block_rows) {
    case 64: hipLaunchKernelGGL((bank_mark_kernel<P, 64>), grid, dim3(64), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 128: hipLaunchKernelGGL((bank_mark_kernel<P, 128>), grid, dim3(128), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    case 256: hipLaunchKernelGGL((bank_mark_kernel<P, 256>), grid, dim3(256), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
    default: hipLaunchKernelGGL((bank_mark_kernel<P, 512>), grid, dim3(512), 0, h->stream, h->U, h->sa, h->vT, h->bv, h->wd, a); break;
  }
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
    h->timed = false;
    HIPCHK(hipEventRecord(h->ev[0], h->stream));
  }
  void done() {
    HIPCHK(hipEventRecord(h->ev[1], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timed = true;
  }
};

}  // namespace

extern "C" {

const char* mvb_last_error(mvb_index* h) { return h ? h->err.c_str() : g_err.c_str(); }

int mvb_create(int device, int proj_dim, const float* Wm, int same_idx, mvb_index** out) try {
  need(out != nullptr, "out is NULL");
  *out = nullptr;
  need(proj_dim == 512 || proj_dim == 768, "proj_dim = " + std::to_string(proj_dim) + ": the matcher runs on 512 or 768 features");
  need(same_idx == 0 || same_idx == 1, "same_idx = " + std::to_string(same_idx) + ": 0 or 1");
  need(Wm != nullptr, "the matcher weight is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MVB_ERR_HIP, "no HIP device: the bank audit has no CPU fallback");
  need(device >= 0 && device < ndev, "device " + std::to_string(device) + " of " + std::to_string(ndev));
  HIPCHK(hipSetDevice(device));
  mvb_index* h = new mvb_index();
  h->device = device; h->P = proj_dim; h->same_idx = same_idx;
  try {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev) HIPCHK(hipEventCreate(&e));
    float* wm = nullptr;
    HIPCHK(hipMalloc((void**)&h->wd, (size_t)3 * h->P * sizeof(float)));
    HIPCHK(hipMalloc((void**)&h->gstate, sizeof(BankGreedyState)));
    HIPCHK(hipMalloc((void**)&wm, (size_t)6 * h->P * sizeof(float)));
    hipError_t e = hipMemcpyAsync(wm, Wm, (size_t)6 * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(bank_weight_delta_kernel, dim3((3 * h->P + 255) / 256), dim3(256), 0, h->stream, wm, h->wd, h->P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(wm);
    hipchk(e, "uploading the matcher weight");
  } catch (...) {
    mvb_destroy(h);
    throw;
  }
  *out = h;
  return MVB_OK;
} catch (...) { return on_exception(nullptr); }

void mvb_destroy(mvb_index* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->cls, (void*)h->wd, (void*)h->vdev, (void*)h->vT, (void*)h->bv, (void*)h->thr, (void*)h->out, (void*)h->mult,
                  (void*)h->sole_of, (void*)h->tiles, (void*)h->taken, (void*)h->part, (void*)h->order, (void*)h->gained, (void*)h->gstate, (void*)h->bits,
                  (void*)h->pos, (void*)h->covered})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int mvb_add(mvb_index* h, const float* embed, int64_t n) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  need(n >= 0, "n = " + std::to_string(n) + " rows");
  need(n <= MVB_MAX_ROWS - h->n, "the index would hold more than 2^31 - 2 rows");
  if (n == 0) return MVB_OK;
  need(embed != nullptr, "the embeddings are NULL");
  HIPCHK(hipSetDevice(h->device));
  reserve_rows(h, h->n + n);
  HIPCHK(hipMemcpyAsync(h->U + (size_t)h->n * h->P, embed, (size_t)n * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->cls + h->n, 0, (size_t)n, h->stream));
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (h->P == 512) hipLaunchKernelGGL(bank_row_term_kernel<512>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  else hipLaunchKernelGGL(bank_row_term_kernel<768>, grid, block, 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  launched("bank_row_term_kernel");
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's buffer is free again, and the rows count only once they are there)
  h->n += n;
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
  need(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  if (n == 0) return MVB_OK;
  need(cls != nullptr, "the classes are NULL");
  for (int64_t i = 0; i < n; ++i) need(cls[i] <= 1, "cls[" + std::to_string(i) + "] = " + std::to_string((int)cls[i]) + ": a class is 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->cls + first, cls, (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_mark(mvb_index* h, const float* v, int Q, const float* thres, int64_t first, int64_t count) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  h->timed = false;
  need(v != nullptr, "the vectors are NULL");
  need(Q >= 1 && Q <= MVB_MAX_VECTORS, "Q = " + std::to_string(Q) + ": 1 <= Q <= 4096");
  need(first >= 0 && count >= 0 && first <= h->n && count <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  need(thres != nullptr, "the thresholds are NULL");
  for (int i = 0; i < Q; ++i) need(std::isfinite(thres[i]), "thres[" + std::to_string(i) + "] is not finite");
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
  grow(h->vdev, h->vdev_n, (size_t)Q * h->P);
  grow(h->thr, h->thr_n, (size_t)Q);
  grow(h->vT, h->vT_n, (size_t)h->P * Qs_max);
  grow(h->bv, h->bv_n, (size_t)Qs_max);
  grow(h->bits, h->bits_n, (size_t)Q * W);
  grow(h->pos, h->pos_n, (size_t)W);
  grow(h->covered, h->covered_n, (size_t)W);
  HIPCHK(hipMemcpyAsync(h->vdev, v, (size_t)Q * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->thr, thres, (size_t)Q * sizeof(float), hipMemcpyHostToDevice, h->stream));
  Timed t(h);
  for (int q0 = 0; q0 < Q; q0 += group) {
    const int nq = std::min(group, Q - q0);
    const int Qs = (nq + BK_QT - 1) / BK_QT * BK_QT;
    const float* vg = h->vdev + (size_t)q0 * h->P;
    if (h->P == 512) hipLaunchKernelGGL(bank_vector_prep_kernel<512>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, vg, h->wd, h->vT, h->bv, nq, Qs);
    else hipLaunchKernelGGL(bank_vector_prep_kernel<768>, dim3((Qs + 63) / 64), dim3(64), 0, h->stream, vg, h->wd, h->vT, h->bv, nq, Qs);
    launched("bank_vector_prep_kernel");
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
    h->timed = false;
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
    h->timed = false;
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
    h->timed = false;
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
    h->timed = false;
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
  need(ms != nullptr, "ms is NULL");
  need(h->timed, "the last call launched no kernel");
  float a = 0.f;
  HIPCHK(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  *ms = a;
  return MVB_OK;
} catch (...) { return on_exception(h); }

int mvb_test_plan(mvb_index* h, int block_rows, int vector_group, int word_chunk) try {
  if (!h) return fail(nullptr, MVB_ERR_ARG, "index is NULL");
  drop_marking(h);
  need(block_rows == 0 || block_rows == 64 || block_rows == 128 || block_rows == 256 || block_rows == 512,
       "block_rows = " + std::to_string(block_rows) + ": 0, 64, 128, 256 or 512");
  need(vector_group >= 0 && vector_group <= MVB_MAX_VECTORS, "vector_group = " + std::to_string(vector_group) + ": 0 .. 4096");
  need(word_chunk >= 0 && word_chunk <= (1 << 24), "word_chunk = " + std::to_string(word_chunk) + ": 0 .. 2^24");
  h->plan_block_rows = block_rows; h->plan_vector_group = vector_group; h->plan_word_chunk = word_chunk;
  return MVB_OK;
} catch (...) { return on_exception(h); }

}  // extern "C"
