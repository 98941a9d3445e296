// The index over a kept corpus that libmemvul_retrieve.so, libmemvul_claims.so, libmemvul_bank.so and libmemvul_rank.so share: the rows and their row terms on the
// device, the error plumbing of the C boundary, and the calls that are the same in all four (create, add, set_classes, the range check, the vectors' upload; kernel_ms
// for the three that time a call by event pairs).  Host code only; retrieve.hip, claims.hip, bank.hip and rank.hip include it and derive their index from KeptIndex,
// adding their own workspace and held state.
//
// Everything here has INTERNAL linkage (one anonymous namespace, no inline function with vague linkage): a process loads the four libraries side by side, and a
// symbol the dynamic linker could bind across them would tie one library's host code to another's (build.py's note on -Bsymbolic records what that cost once).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace {

// the return codes and limits the four public headers share; each library asserts its own macros against them
constexpr int KEPT_OK = 0, KEPT_ERR_ARG = -1, KEPT_ERR_HIP = -2, KEPT_ERR_NOMEM = -3, KEPT_ERR_INTERNAL = -4, KEPT_ERR_STATE = -5;
constexpr int KEPT_MAX_VECTORS = 4096;
constexpr int64_t KEPT_MAX_ROWS = 2147483646ll;
#define KEPT_ASSERT_ABI(PFX, MAX_VECTORS)                                                                                                           \
  static_assert(PFX##_OK == KEPT_OK && PFX##_ERR_ARG == KEPT_ERR_ARG && PFX##_ERR_HIP == KEPT_ERR_HIP && PFX##_ERR_NOMEM == KEPT_ERR_NOMEM &&       \
                    PFX##_ERR_INTERNAL == KEPT_ERR_INTERNAL && PFX##_MAX_ROWS == KEPT_MAX_ROWS && MAX_VECTORS == KEPT_MAX_VECTORS,                  \
                "the public header and kept_index.h disagree")

// the kernels of kept_terms.h under the names the including library gives them
struct KeptKernels {
  void (*weight_delta)(const float*, float*, int);
  void (*row_term[2])(const float*, const float*, float*, long long, long long);       // P = 512, 768
  void (*vector_prep[2])(const float*, const float*, float*, float*, int, int);        // P = 512, 768
};

struct KeptIndex {
  const KeptKernels* kernels;
  const bool has_cls;                 // the rows carry a class byte (the retrieval index allocates none)
  const int nev;                      // events created: two per pair (none for the ranking index, whose stage clock keeps its own)
  int device = 0, P = 0, same_idx = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // ev[0..1] bracket the launches of a call, ev[2..3] those of a call's second phase
  int timed = 0;                      // event pairs to add up
  float *U = nullptr, *sa = nullptr;  // rows [cap][P], row terms [cap]
  uint8_t* cls = nullptr;             // [cap]
  int64_t n = 0, cap = 0;
  float* wd = nullptr;                // [3][P] class-difference weights
  // workspace (grows, never shrinks)
  float *vdev = nullptr, *vT = nullptr, *bv = nullptr;  // the vectors [Q][P]; one group transposed [P][Qs]; its bv [Qs]
  size_t vdev_n = 0, vT_n = 0, bv_n = 0;
  std::string err;
  KeptIndex(const KeptKernels* k, bool has_cls_, int nev_) : kernels(k), has_cls(has_cls_), nev(nev_) {}
};

thread_local std::string g_err;  // errors with no index to hang them on (create)

struct Refusal : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct StateError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(KeptIndex* h, int code, const std::string& msg) {
  (h ? h->err : g_err) = msg;
  return code;
}

int on_exception(KeptIndex* h) noexcept {
  try {
    try {
      throw;
    } catch (const Refusal& e) {
      return fail(h, KEPT_ERR_ARG, e.what());
    } catch (const StateError& e) {
      return fail(h, KEPT_ERR_STATE, e.what());
    } catch (const std::bad_alloc&) {
      return fail(h, KEPT_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
      return fail(h, KEPT_ERR_HIP, e.what());
    } catch (...) {
      return fail(h, KEPT_ERR_INTERNAL, "unknown C++ exception");
    }
  } catch (...) {  // (the message itself could not be stored)
    return KEPT_ERR_INTERNAL;
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

void reserve_rows(KeptIndex* h, int64_t want) {
  if (want <= h->cap) return;
  const int64_t cap = std::max<int64_t>(want, std::min<int64_t>(h->cap + h->cap / 2, KEPT_MAX_ROWS));
  float *U = nullptr, *sa = nullptr;
  uint8_t* cls = nullptr;
  hipError_t e = hipMalloc((void**)&U, (size_t)cap * h->P * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&sa, (size_t)cap * sizeof(float));
  if (e == hipSuccess && h->has_cls) e = hipMalloc((void**)&cls, (size_t)cap);
  if (e == hipSuccess && h->n) {
    e = hipMemcpyAsync(U, h->U, (size_t)h->n * h->P * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sa, h->sa, (size_t)h->n * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess && h->has_cls) e = hipMemcpyAsync(cls, h->cls, (size_t)h->n, hipMemcpyDeviceToDevice, h->stream);
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

// the body of mvX_create.  noun: what the "no CPU fallback" message calls the index; destroy: mvX_destroy; init: what the library allocates at creation beyond the base
template <class Index, class Init = void (*)(Index*)>
void kept_create(const char* noun, void (*destroy)(Index*), int device, int proj_dim, const float* Wm, int same_idx, Index** out, Init init = [](Index*) {}) {
  need(out != nullptr, "out is NULL");
  *out = nullptr;
  need(proj_dim == 512 || proj_dim == 768, "proj_dim = " + std::to_string(proj_dim) + ": the matcher runs on 512 or 768 features");
  need(same_idx == 0 || same_idx == 1, "same_idx = " + std::to_string(same_idx) + ": 0 or 1");
  need(Wm != nullptr, "the matcher weight is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw std::runtime_error(std::string("no HIP device: the ") + noun + " has no CPU fallback");
  need(device >= 0 && device < ndev, "device " + std::to_string(device) + " of " + std::to_string(ndev));
  HIPCHK(hipSetDevice(device));
  Index* h = new Index();
  h->device = device; h->P = proj_dim; h->same_idx = same_idx;
  try {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (int i = 0; i < h->nev; ++i) HIPCHK(hipEventCreate(&h->ev[i]));
    float* wm = nullptr;
    HIPCHK(hipMalloc((void**)&h->wd, (size_t)3 * h->P * sizeof(float)));
    init(h);
    HIPCHK(hipMalloc((void**)&wm, (size_t)6 * h->P * sizeof(float)));
    hipError_t e = hipMemcpyAsync(wm, Wm, (size_t)6 * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(h->kernels->weight_delta, dim3((3 * h->P + 255) / 256), dim3(256), 0, h->stream, wm, h->wd, h->P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(wm);
    hipchk(e, "uploading the matcher weight");
  } catch (...) {
    destroy(h);
    throw;
  }
  *out = h;
}

// everything of mvX_destroy but the delete.  own: the buffers the library holds beyond the base
void kept_destroy_common(KeptIndex* h, std::initializer_list<void*> own) {
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->U, (void*)h->sa, (void*)h->cls, (void*)h->wd, (void*)h->vdev, (void*)h->vT, (void*)h->bv})
    if (p) (void)hipFree(p);
  for (void* p : own)
    if (p) (void)hipFree(p);
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

void kept_add(KeptIndex* h, const float* embed, int64_t n) {
  need(n >= 0, "n = " + std::to_string(n) + " rows");
  need(n <= KEPT_MAX_ROWS - h->n, "the index would hold more than 2^31 - 2 rows");
  if (n == 0) return;
  need(embed != nullptr, "the embeddings are NULL");
  HIPCHK(hipSetDevice(h->device));
  reserve_rows(h, h->n + n);
  HIPCHK(hipMemcpyAsync(h->U + (size_t)h->n * h->P, embed, (size_t)n * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (h->has_cls) HIPCHK(hipMemsetAsync(h->cls + h->n, 0, (size_t)n, h->stream));
  hipLaunchKernelGGL(h->kernels->row_term[h->P == 768], dim3((unsigned)((n + 3) / 4)), dim3(256), 0, h->stream, h->U, h->wd, h->sa, (long long)h->n, (long long)n);
  launched("the row-term kernel");
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's buffer is free again, and the rows count only once they are there)
  h->n += n;
}

void kept_set_classes(KeptIndex* h, const uint8_t* cls, int64_t first, int64_t n) {
  need(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") are not within the " + std::to_string(h->n) + " rows of the index");
  if (n == 0) return;
  need(cls != nullptr, "the classes are NULL");
  for (int64_t i = 0; i < n; ++i) need(cls[i] <= 1, "cls[" + std::to_string(i) + "] = " + std::to_string((int)cls[i]) + ": a class is 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(h->cls + first, cls, (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
}

// vectors: what the refusal of a NULL pointer calls them ("vectors", "query vectors")
void check_range(const KeptIndex* h, const char* vectors, const float* v, int Q, int64_t first, int64_t count) {
  need(v != nullptr, std::string("the ") + vectors + " are NULL");
  need(Q >= 1 && Q <= KEPT_MAX_VECTORS, "Q = " + std::to_string(Q) + ": 1 <= Q <= 4096");
  need(first >= 0 && count >= 0 && first <= h->n && count <= h->n - first,
       "rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(count) + ") are not within the " + std::to_string(h->n) + " rows of the index");
}

void check_thresholds(const float* thres, int n) {
  need(thres != nullptr, "the thresholds are NULL");
  for (int i = 0; i < n; ++i) need(std::isfinite(thres[i]), "thres[" + std::to_string(i) + "] is not finite");
}

void check_block_rows(int block_rows) {
  need(block_rows == 0 || block_rows == 64 || block_rows == 128 || block_rows == 256 || block_rows == 512,
       "block_rows = " + std::to_string(block_rows) + ": 0, 64, 128, 256 or 512");
}

void kept_upload_vectors(KeptIndex* h, const float* v, int Q) {
  grow(h->vdev, h->vdev_n, (size_t)Q * h->P);
  HIPCHK(hipMemcpyAsync(h->vdev, v, (size_t)Q * h->P * sizeof(float), hipMemcpyHostToDevice, h->stream));
}

// the group's vectors [q0, q0 + nq) of vdev transposed to vT [P][Qs], and their bv
void kept_vector_prep(KeptIndex* h, int q0, int nq, int Qs) {
  hipLaunchKernelGGL(h->kernels->vector_prep[h->P == 768], dim3((Qs + 63) / 64), dim3(64), 0, h->stream, h->vdev + (size_t)q0 * h->P, h->wd, h->vT, h->bv, nq, Qs);
  launched("the vector-prep kernel");
}

// none: the refusal when the last call launched nothing
void kept_kernel_ms(KeptIndex* h, float* ms, const char* none) {
  need(ms != nullptr, "ms is NULL");
  need(h->timed > 0, none);
  float sum = 0.f;
  for (int pair = 0; pair < h->timed; ++pair) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, h->ev[2 * pair], h->ev[2 * pair + 1]));
    sum += t;
  }
  *ms = sum;
}

// launch(std::integral_constant<int, BR>) for the rows per block of a score / mark kernel: 64, 128, 256, or 512
template <class Launch>
void by_block_rows(int block_rows, Launch launch) {
  switch (block_rows) {
    case 64: launch(std::integral_constant<int, 64>{}); break;
    case 128: launch(std::integral_constant<int, 128>{}); break;
    case 256: launch(std::integral_constant<int, 256>{}); break;
    default: launch(std::integral_constant<int, 512>{}); break;
  }
}

}  // namespace
