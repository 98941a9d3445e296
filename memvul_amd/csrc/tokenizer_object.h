// Part of engine.hip: the device WordPiece tokenizer as an object of its own (mv_tokenizer, tok_*, the mv_tok_* entries; the kernel: wordpiece.h).
// It names no mv_handle beyond the on_exception overloads.

// =================================================================================================
// The device WordPiece tokenizer (include/memvul_hip.h mv_tok_*; memvul_amd/csrc/wordpiece.h): an object of its own — its table, its stream, its buffers —
// that shares no mutable state with any mv_handle, so the tokenising thread may be inside mv_tok_encode while another thread is inside a handle's sweep.
// the UTF-8 kernel's launch, in libmemvul_tok_u8.so (wordpiece_u8.hip): the kernel is kept out of this library's code object
extern "C" int wp_u8_launch(const WpTable* t, const WpU8* u, const uint8_t* text, const int64_t* off, int m, int max_length, int add_special, int32_t* ids,
                            int32_t* lens, uint8_t* status, hipStream_t stream);

struct mv_tokenizer {
  int device = -1;  // < 0: the table only (mv_tok_encode_host)
  WpHost host;
  WpTable dev{};    // the same table with device pointers
  hipStream_t stream = nullptr;
  void *d_slots = nullptr, *d_pool = nullptr, *d_lit = nullptr, *d_lit_off = nullptr;
  std::vector<WpCp> cp;       // mv_tok_set_unicode: the code-point table; empty = the ASCII rule only
  WpU8 u8_host{}, u8_dev{};   // what the UTF-8 drivers take beside the table (host pointers / device pointers)
  void* d_cp = nullptr;
  void *d_text = nullptr, *d_off = nullptr, *d_ids = nullptr, *d_lens = nullptr, *d_status = nullptr;  // grow to the largest call
  size_t cap_text = 0, cap_off = 0, cap_ids = 0, cap_lens = 0, cap_status = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around each chunk's kernel
  float kernel_ms = 0.f;                    // the kernel's own time over the chunks of the last mv_tok_encode / mv_tok_encode_u8 (mv_tok_kernel_ms)
  std::vector<int64_t> rel;  // a chunk's offsets, rebased to its first byte
  std::string err;
};

namespace {

int tok_fail(mv_tokenizer* t, int code, const std::string& msg) {
  if (t) t->err = msg; else g_create_error = msg;
  return code;
}

int on_exception(std::nullptr_t) noexcept { return on_exception((mv_handle*)nullptr); }  // (the entries without an object: not ambiguous between the two below)

int on_exception(mv_tokenizer* t) noexcept {
  const int code = on_exception((mv_handle*)nullptr);  // (classifies the exception in flight; the message lands in g_create_error)
  try {
    if (t) t->err = g_create_error;
  } catch (...) {
  }
  return code;
}

#define TOKHIP(t, expr)                                                                              \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return tok_fail(t, MV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)

constexpr int64_t kTokChunkBytes = 64ll << 20;  // text per launch
constexpr int kTokChunkRows = 1 << 16;          // rows per launch: bounds the id buffer at 128 MiB

// what mv_tok_encode*, all four, refuse before they touch an output
int tok_check_args(mv_tokenizer* tok, const char* what, const char* text, const int64_t* off, int n, int max_length, const int32_t* ids, const int32_t* lens,
                   const uint8_t* status) {
  if (n < 0 || max_length < 2 || max_length > WP_MAX_LENGTH) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": n < 0 or max_length outside 2 .. 512");
  if (n == 0) return MV_OK;
  if (!off || !ids || !lens || !status) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": NULL offsets or output");
  if (off[0] < 0) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": negative offset");
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": offsets not ascending");
  if (off[n] > off[0] && !text) return tok_fail(tok, MV_ERR_INVALID, std::string(what) + ": NULL text");
  return MV_OK;
}

int tok_grow(mv_tokenizer* tok, void** p, size_t* cap, size_t need) {
  if (need <= *cap) return MV_OK;
  if (*p) TOKHIP(tok, hipFree(*p));
  *p = nullptr;
  *cap = 0;
  const size_t want = (need + need / 4 + 255) & ~(size_t)255;
  if (hipMalloc(p, want) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return tok_fail(tok, MV_ERR_NOMEM, "mv_tok_encode: device allocation of " + std::to_string(want) + " bytes failed");
  }
  *cap = want;
  return MV_OK;
}

void tok_release(mv_tokenizer* t) {
  if (t->device >= 0 && hipSetDevice(t->device) == hipSuccess) {
    if (t->stream) hipStreamSynchronize(t->stream);
    for (void* p : {t->d_slots, t->d_pool, t->d_lit, t->d_lit_off, t->d_cp, t->d_text, t->d_off, t->d_ids, t->d_lens, t->d_status})
      if (p) hipFree(p);
    if (t->ev0) hipEventDestroy(t->ev0);
    if (t->ev1) hipEventDestroy(t->ev1);
    if (t->stream) hipStreamDestroy(t->stream);
  }
  delete t;
}

// the chunks of one mv_tok_encode / mv_tok_encode_u8 call (u8: the UTF-8 kernel), enqueued and collected one after the other on the object's stream
int tok_encode_chunks(mv_tokenizer* tok, bool u8, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                      uint8_t* status) {
  for (int r0 = 0; r0 < n;) {
    // a chunk ends before the row that would take it past 64 MiB of text (a single larger row is a chunk of its own) and after 65 536 rows
    int r1 = r0 + 1;
    while (r1 < n && r1 - r0 < kTokChunkRows && off[r1 + 1] - off[r0] <= kTokChunkBytes) ++r1;
    const int m = r1 - r0;
    const int64_t bytes = off[r1] - off[r0];
    if (int rc = tok_grow(tok, &tok->d_text, &tok->cap_text, (size_t)bytes + 1)) return rc;
    if (int rc = tok_grow(tok, &tok->d_off, &tok->cap_off, (size_t)(m + 1) * sizeof(int64_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_ids, &tok->cap_ids, (size_t)m * max_length * sizeof(int32_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_lens, &tok->cap_lens, (size_t)m * sizeof(int32_t))) return rc;
    if (int rc = tok_grow(tok, &tok->d_status, &tok->cap_status, (size_t)m)) return rc;
    tok->rel.resize((size_t)m + 1);
    for (int i = 0; i <= m; ++i) tok->rel[i] = off[r0 + i] - off[r0];
    if (bytes > 0) TOKHIP(tok, hipMemcpyAsync(tok->d_text, text + off[r0], (size_t)bytes, hipMemcpyHostToDevice, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(tok->d_off, tok->rel.data(), (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, tok->stream));
    TOKHIP(tok, hipEventRecord(tok->ev0, tok->stream));
    if (u8) {
      TOKHIP(tok, (hipError_t)wp_u8_launch(&tok->dev, &tok->u8_dev, (const uint8_t*)tok->d_text, (const int64_t*)tok->d_off, m, max_length, add_special ? 1 : 0,
                                           (int32_t*)tok->d_ids, (int32_t*)tok->d_lens, (uint8_t*)tok->d_status, tok->stream));
    } else {
      hipLaunchKernelGGL(wp_encode_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, tok->stream, tok->dev, (const uint8_t*)tok->d_text,
                         (const int64_t*)tok->d_off, m, max_length, add_special ? 1 : 0, (int32_t*)tok->d_ids, (int32_t*)tok->d_lens, (uint8_t*)tok->d_status);
      TOKHIP(tok, hipGetLastError());
    }
    TOKHIP(tok, hipEventRecord(tok->ev1, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(ids + (size_t)r0 * max_length, tok->d_ids, (size_t)m * max_length * sizeof(int32_t), hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(lens + r0, tok->d_lens, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipMemcpyAsync(status + r0, tok->d_status, (size_t)m, hipMemcpyDeviceToHost, tok->stream));
    TOKHIP(tok, hipStreamSynchronize(tok->stream));
    float ms = 0.f;
    TOKHIP(tok, hipEventElapsedTime(&ms, tok->ev0, tok->ev1));
    tok->kernel_ms += ms;
    r0 = r1;
  }
  return MV_OK;
}

// mv_tok_encode and mv_tok_encode_u8 behind their checks
int tok_encode_device(mv_tokenizer* tok, const char* what, bool u8, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids,
                      int32_t* lens, uint8_t* status) {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, std::string(what) + ": tok is NULL");
  if (int rc = tok_check_args(tok, what, text, off, n, max_length, ids, lens, status)) return rc;
  if (n == 0) return MV_OK;
  if (u8 && tok->cp.empty()) return tok_fail(tok, MV_ERR_STATE, std::string(what) + ": no code-point table (mv_tok_set_unicode)");
  if (tok->device < 0) return tok_fail(tok, MV_ERR_STATE, std::string(what) + ": created without a device (mv_tok_create(device < 0) serves the _host entries)");
  TOKHIP(tok, hipSetDevice(tok->device));
  tok->kernel_ms = 0.f;
  const int rc = tok_encode_chunks(tok, u8, text, off, n, max_length, add_special, ids, lens, status);
  if (rc != MV_OK) (void)hipStreamSynchronize(tok->stream);  // nothing queued on the stream writes the caller's arrays after the call has failed
  return rc;
}

}  // namespace

extern "C" {

// ---- the device WordPiece tokenizer ------------------------------------------------------------------------------------------------------------------------------
int mv_tok_create(int device, const char* vocab_bytes, const int64_t* vocab_off, int n_vocab, const char* literal_bytes, const int64_t* literal_off,
                  int n_literals, int unk_id, int cls_id, int sep_id, int max_chars_per_word, int lowercase, mv_tokenizer** out) try {
  if (!out) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_create: out is NULL");
  *out = nullptr;
  mv_tokenizer* t = new mv_tokenizer();
  struct Guard {  // whatever leaves this function early, an exception included, releases the object
    mv_tokenizer* t;
    ~Guard() { if (t) tok_release(t); }
  } guard{t};
  std::string err;
  if (!wp_build(t->host, vocab_bytes, vocab_off, n_vocab, literal_bytes, literal_off, n_literals, unk_id, cls_id, sep_id, max_chars_per_word, lowercase, err))
    return tok_fail(nullptr, MV_ERR_INVALID, err);
  if (device >= 0) {
    t->device = device;
    const WpHost& H = t->host;
    auto up = [&](void** d, const void* src, size_t bytes) -> hipError_t {
      hipError_t e = hipMalloc(d, bytes);
      return e != hipSuccess ? e : hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice);
    };
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&t->ev0);
    if (e == hipSuccess) e = hipEventCreate(&t->ev1);
    if (e == hipSuccess) e = up(&t->d_slots, H.slots.data(), H.slots.size() * sizeof(WpSlot));
    if (e == hipSuccess) e = up(&t->d_pool, H.pool.data(), H.pool.size());
    if (e == hipSuccess) e = up(&t->d_lit, H.lit.data(), H.lit.size());
    if (e == hipSuccess) e = up(&t->d_lit_off, H.lit_off.data(), H.lit_off.size() * sizeof(uint32_t));
    if (e != hipSuccess) {
      const std::string msg = std::string("mv_tok_create: ") + hipGetErrorString(e);
      (void)hipGetLastError();
      return tok_fail(nullptr, MV_ERR_HIP, msg);
    }
    t->dev = H.t;
    t->dev.slots = (const WpSlot*)t->d_slots;
    t->dev.pool = (const uint8_t*)t->d_pool;
    t->dev.lit = (const uint8_t*)t->d_lit;
    t->dev.lit_off = (const uint32_t*)t->d_lit_off;
  }
  guard.t = nullptr;
  *out = t;
  return MV_OK;
} catch (...) { return on_exception((mv_tokenizer*)nullptr); }

void mv_tok_destroy(mv_tokenizer* tok) {
  if (tok) tok_release(tok);
}

const char* mv_tok_last_error(mv_tokenizer* tok) { return tok ? tok->err.c_str() : g_create_error.c_str(); }

int mv_tok_encode_host(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                       uint8_t* status) try {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_encode_host: tok is NULL");
  if (int rc = tok_check_args(tok, "mv_tok_encode_host", text, off, n, max_length, ids, lens, status)) return rc;
  for (int i = 0; i < n; ++i)
    wp_encode_text(tok->host.t, (const uint8_t*)text + off[i], off[i + 1] - off[i], max_length, add_special, ids + (size_t)i * max_length, lens + i, status + i);
  return MV_OK;
} catch (...) { return on_exception(tok); }

int mv_tok_encode(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                  uint8_t* status) try {
  return tok_encode_device(tok, "mv_tok_encode", false, text, off, n, max_length, add_special, ids, lens, status);
} catch (...) { return on_exception(tok); }

// ---- UTF-8: the code-point table and the two entries that use it ----------------------------------------------------------------------------------------------------
int mv_tok_set_unicode(mv_tokenizer* tok, const void* entries, int n_entries) try {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_set_unicode: tok is NULL");
  static_assert(sizeof(WpCp) == 16, "the code-point table's entries are 16 bytes");
  std::string err;
  if (!wp_u8_check_table((const WpCp*)entries, n_entries, tok->host.t.max_chars, err)) return tok_fail(tok, MV_ERR_INVALID, err);
  std::vector<WpCp> cp((const WpCp*)entries, (const WpCp*)entries + n_entries);
  void* d_new = nullptr;
  if (tok->device >= 0) {  // the new table is on the device before the old one goes: a failed call leaves the object as it was
    TOKHIP(tok, hipSetDevice(tok->device));
    TOKHIP(tok, hipStreamSynchronize(tok->stream));
    if (hipMalloc(&d_new, cp.size() * sizeof(WpCp)) != hipSuccess) {
      (void)hipGetLastError();
      return tok_fail(tok, MV_ERR_NOMEM, "mv_tok_set_unicode: device allocation of the code-point table failed");
    }
    const hipError_t e = hipMemcpy(d_new, cp.data(), cp.size() * sizeof(WpCp), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d_new);
      return tok_fail(tok, MV_ERR_HIP, std::string("mv_tok_set_unicode: ") + hipGetErrorString(e));
    }
    if (tok->d_cp) (void)hipFree(tok->d_cp);
    tok->d_cp = d_new;
  }
  tok->cp.swap(cp);
  tok->u8_host = WpU8{tok->cp.data(), n_entries, tok->host.max_len0_all, tok->host.max_len1_all, tok->host.lit_first2, tok->host.lit_first3};
  tok->u8_dev = WpU8{(const WpCp*)tok->d_cp, n_entries, tok->host.max_len0_all, tok->host.max_len1_all, tok->host.lit_first2, tok->host.lit_first3};
  return MV_OK;
} catch (...) { return on_exception(tok); }

int mv_tok_encode_u8_host(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                          uint8_t* status) try {
  if (!tok) return tok_fail(nullptr, MV_ERR_INVALID, "mv_tok_encode_u8_host: tok is NULL");
  if (int rc = tok_check_args(tok, "mv_tok_encode_u8_host", text, off, n, max_length, ids, lens, status)) return rc;
  if (n == 0) return MV_OK;
  if (tok->cp.empty()) return tok_fail(tok, MV_ERR_STATE, "mv_tok_encode_u8_host: no code-point table (mv_tok_set_unicode)");
  for (int i = 0; i < n; ++i)
    wp_encode_text_u8(tok->host.t, tok->u8_host, (const uint8_t*)text + off[i], off[i + 1] - off[i], max_length, add_special, ids + (size_t)i * max_length, lens + i,
                      status + i);
  return MV_OK;
} catch (...) { return on_exception(tok); }

int mv_tok_encode_u8(mv_tokenizer* tok, const char* text, const int64_t* off, int n, int max_length, int add_special, int32_t* ids, int32_t* lens,
                     uint8_t* status) try {
  return tok_encode_device(tok, "mv_tok_encode_u8", true, text, off, n, max_length, add_special, ids, lens, status);
} catch (...) { return on_exception(tok); }

int mv_tok_kernel_ms(mv_tokenizer* tok, float* ms) try {
  if (!tok || !ms) return tok_fail(tok, MV_ERR_INVALID, "mv_tok_kernel_ms: NULL argument");
  *ms = tok->kernel_ms;
  return MV_OK;
} catch (...) { return on_exception(tok); }

}  // extern "C"
