// Part of engine.hip: what every other part stands on — error reporting (fail, on_exception, HIPCHK), device memory owned by a handle (dev_alloc / dev_free),
// the profiling events (ProfScope), launch_check, the fp16 / bf16 bit conversions, and the waits and input checks the entry points open with.

namespace {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// fp32 -> fp16 bits, round-to-nearest-even (same result as numpy astype(float16))
inline uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520 -> inf
  if (x < 0x38800000u) {                                     // subnormal half or zero
    if (x < 0x33000000u) return (uint16_t)sign;              // < 2^-25 -> 0
    const int e = (int)(x >> 23);
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;  // 14..24 -> bits to drop
    const uint32_t half_m = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    uint32_t r = half_m;
    if (rem > halfway || (rem == halfway && (half_m & 1))) r++;
    return (uint16_t)(sign | r);
  }
  const uint32_t e = (x >> 23) - 112, m = x & 0x7fffffu;
  uint32_t h = (e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) h++;
  return (uint16_t)(sign | h);
}
inline float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, x;
  if (e == 0) {
    if (m == 0) x = sign;
    else {
      int sh = 0;
      while (!(m & 0x400u)) { m <<= 1; sh++; }
      m &= 0x3ffu;
      x = sign | ((uint32_t)(113 - sh) << 23) | (m << 13);
    }
  } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
  else x = sign | ((e + 112) << 23) | (m << 13);
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}
inline float bf16_bits_to_f32(uint16_t h) {
  uint32_t x = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}

int fail(mv_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

// No C++ exception crosses the ABI (include/memvul_hip.h): every entry point is a function-try-block whose handler lands here
// (std::bad_alloc of the host-side staging vectors / maps -> MV_ERR_NOMEM, anything else -> MV_ERR_INTERNAL).
int on_exception(mv_handle* h) noexcept {
  int code = MV_ERR_INTERNAL;
  const char* what = "unknown C++ exception";
  try {
    throw;
  } catch (const std::bad_alloc&) {
    code = MV_ERR_NOMEM;
    what = "out of host memory";
  } catch (const std::exception& e) {
    what = e.what();
  } catch (...) {
  }
  try {
    fail(h, code, std::string("internal: ") + what);
  } catch (...) {  // not even the message could be stored
  }
  return code;
}

#define HIPCHK(h, expr)                                                                             \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return fail(h, MV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

template <typename T>
int dev_alloc(mv_handle* h, hipStream_t stream, T** p, int64_t count, bool zero = true) {
  void* d = nullptr;
  const size_t bytes = (size_t)count * sizeof(T);
  hipError_t e = hipMalloc(&d, bytes ? bytes : 16);
  if (e != hipSuccess) return fail(h, MV_ERR_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  if (zero) {
    e = hipMemsetAsync(d, 0, bytes ? bytes : 16, stream);
    if (e != hipSuccess) return fail(h, MV_ERR_HIP, std::string("hipMemset failed: ") + hipGetErrorString(e));
  }
  h->allocs.push_back(d);
  *p = (T*)d;
  return MV_OK;
}
void dev_free(mv_handle* h, void* p) {
  if (!p) return;
  for (auto it = h->allocs.begin(); it != h->allocs.end(); ++it)
    if (*it == p) { h->allocs.erase(it); break; }
  hipFree(p);
}

hipEvent_t get_event(mv_handle* h) {
  if (!h->free_events.empty()) {
    hipEvent_t e = h->free_events.back();
    h->free_events.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

struct ProfScope {
  mv_handle* h;
  hipStream_t stream;
  ProfRec rec;
  bool on;
  ProfScope(mv_handle* h_, hipStream_t s, int cls) : h(h_), stream(s), on(h_->prof && ((h_->prof_mask >> cls) & 1u)) {
    if (on) {
      rec.cls = cls;
      rec.e0 = get_event(h);
      rec.e1 = get_event(h);
      hipEventRecord(rec.e0, stream);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(rec.e1, stream);
      h->recs.push_back(rec);
    }
  }
};

int launch_check(mv_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, MV_ERR_HIP, std::string("launch ") + what + ": " + hipGetErrorString(e));
  return MV_OK;
}

int sync_all(mv_handle* h) {  // (a ticket stays in flight until mv_forward_ragged_end collects it)
  for (int wi = 0; wi < h->n_alloc; ++wi) { HIPCHK(h, hipStreamSynchronize(h->work[wi].stream)); h->work[wi].sweep = false; }
  return MV_OK;
}

int check_final(mv_handle* h) {
  if (!h) return MV_ERR_INVALID;
  if (!h->finalized) return fail(h, MV_ERR_STATE, "weights not finalized (mv_finalize_weights)");
  return MV_OK;
}

// Every entry point but the resident sweep works on set 0 (mv_forward_ragged_begin: on a set without a ticket), stream-ordered behind
// what is there; a sweep may have left the other set busy (it reads the anchor bank and the resident corpus): wait for it first.
int check_ready(mv_handle* h) {
  if (int rc = check_final(h)) return rc;
  for (int wi = 1; wi < h->n_alloc; ++wi)
    if (h->work[wi].sweep) {
      HIPCHK(h, hipStreamSynchronize(h->work[wi].stream));
      h->work[wi].sweep = false;
    }
  return MV_OK;
}

// HF's embedding lookup raises on an id outside the table; the embedding kernel would clamp silently (a tokenizer /
// checkpoint vocabulary mismatch would then score garbage without a sign): reject such input at the boundary.
int check_ids(mv_handle* h, const int32_t* ids, int64_t n, const char* who) {
  const int32_t V = h->cfg.vocab_size;
  uint32_t bad = 0;
  for (int64_t i = 0; i < n; ++i) bad |= (uint32_t)(ids[i] < 0) | (uint32_t)(ids[i] >= V);
  if (bad) return fail(h, MV_ERR_INVALID, std::string(who) + ": token id outside [0, vocab_size) — tokenizer and checkpoint vocabularies differ?");
  return MV_OK;
}

}  // namespace
