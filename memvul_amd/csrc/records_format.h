// Part of engine.hip: the JSON-lines record formatter (mv_format_records) — host only, no handle, no HIP call.

extern "C" {

// ---- JSON-lines records of one batch (host only) --------------------------------------------------------------------------------------
// Python's repr(float) — what json.dumps prints for every probability of make_output_human_readable's records (model_memory.py:169-191 ->
// predict_memory.py:111) — restated: the shortest digit string that round-trips the double (std::to_chars, scientific) laid out by CPython's rule
// (PyOS_double_to_string 'r': exponent form when the decimal exponent is < -4 or >= 16, at least two exponent digits, ".0" after a whole number).
// 0.65 us per double in CPython, ~40 ns here; pinned to repr() on millions of values by tests/test_host_logic.py.
static inline char* py_repr_double(char* o, double v) {
  if (v == 0.0) {
    if (std::signbit(v)) *o++ = '-';
    *o++ = '0'; *o++ = '.'; *o++ = '0';
    return o;
  }
  char b[40];
  const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::scientific);  // [-]d[.ddd]e[+-]XX
  const char* p = b;
  if (*p == '-') *o++ = *p++;
  char dig[24];
  int nd = 0;
  dig[nd++] = *p++;
  if (*p == '.') {
    ++p;
    while (*p != 'e') dig[nd++] = *p++;
  }
  ++p;  // 'e'
  const bool eneg = *p == '-';
  ++p;
  int e = 0;
  while (p < r.ptr) e = e * 10 + (*p++ - '0');
  if (eneg) e = -e;
  if (e < -4 || e >= 16) {
    *o++ = dig[0];
    if (nd > 1) {
      *o++ = '.';
      for (int i = 1; i < nd; ++i) *o++ = dig[i];
    }
    *o++ = 'e';
    *o++ = e < 0 ? '-' : '+';
    const int ae = e < 0 ? -e : e;
    if (ae >= 100) *o++ = (char)('0' + ae / 100);
    *o++ = (char)('0' + (ae / 10) % 10);
    *o++ = (char)('0' + ae % 10);
  } else if (e < 0) {
    *o++ = '0'; *o++ = '.';
    for (int i = 0; i < -e - 1; ++i) *o++ = '0';
    for (int i = 0; i < nd; ++i) *o++ = dig[i];
  } else {
    for (int i = 0; i <= e; ++i) *o++ = i < nd ? dig[i] : '0';
    *o++ = '.';
    if (nd > e + 1) for (int i = e + 1; i < nd; ++i) *o++ = dig[i];
    else *o++ = '0';
  }
  return o;
}

// out = "[" + ", ".join(prefix_i + piece_0 + repr(p[i][0]) + piece_1 + repr(p[i][1]) + ... + row_suffix) + "]"
int mv_format_records(const char* prefixes, const int64_t* prefix_off, int64_t rows, const char* pieces, const int64_t* piece_off, int64_t cols,
                      const char* row_suffix, const double* p, char* out, int64_t cap, int64_t* written) try {
  if (!prefixes || !prefix_off || !pieces || !piece_off || !row_suffix || !p || !out || !written || rows < 0 || cols < 0) return MV_ERR_INVALID;
  const int64_t nsuf = (int64_t)std::strlen(row_suffix);
  const int64_t piece_bytes = piece_off[cols] - piece_off[0];
  char* o = out;
  char* const end = out + cap;
  if (end - o < 2) return MV_ERR_CAPACITY;
  *o++ = '[';
  for (int64_t i = 0; i < rows; ++i) {
    const int64_t np_ = prefix_off[i + 1] - prefix_off[i];
    if (end - o < np_ + piece_bytes + cols * 26 + nsuf + 4) return MV_ERR_CAPACITY;  // (a repr is at most 24 characters)
    if (i) { *o++ = ','; *o++ = ' '; }
    std::memcpy(o, prefixes + prefix_off[i], (size_t)np_);
    o += np_;
    const double* row = p + i * cols;
    for (int64_t c = 0; c < cols; ++c) {
      const int64_t n = piece_off[c + 1] - piece_off[c];
      std::memcpy(o, pieces + piece_off[c], (size_t)n);
      o += n;
      if (!std::isfinite(row[c])) return MV_ERR_INVALID;  // json spells these NaN / Infinity: the caller's Python path does
      o = py_repr_double(o, row[c]);
    }
    std::memcpy(o, row_suffix, (size_t)nsuf);
    o += nsuf;
  }
  *o++ = ']';
  *written = o - out;
  return MV_OK;
} catch (...) { return on_exception(nullptr); }

}  // extern "C"
