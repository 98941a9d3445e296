// WordPiece for ASCII text (include/memvul_hip.h mv_tok_*): what BertTokenizerFast's backend — BertNormalizer(clean_text), BertPreTokenizer, WordPiece("##"),
// [CLS] A [SEP], truncation on the right — computes for a text whose bytes are all below 0x80, restated exactly.
//
// THE RULE
//   clean      bytes 0-8, 11, 12, 14-31 and 127 are removed (their neighbours join: "ab\x01ab" is the word "abab"); 9, 10, 13 and 32 are whitespace.
//   lower      A-Z -> a-z when the normalizer lower-cases (accent stripping and the CJK rule cannot fire below 0x80).
//   split      on whitespace; every punctuation byte (33-47, 58-64, 91-96, 123-126) is a word of its own.
//   WordPiece  per word the longest vocabulary entry from the left, greedily; pieces after the first are looked up as continuations ("##" entries); a word of
//              more than max_chars bytes, or one with an unmatched remainder, is ONE [UNK].
//   specials   [CLS] first and [SEP] last when asked for; truncation keeps the first max_length - 2 tokens (max_length without specials).  The scan stops
//              tokenising once that budget is full — later tokens are dropped anyway — and only then; there is no cap on the bytes read before that.
//   not ours   a row with a byte >= 0x80, or with one of the tokenizer's added tokens as a literal, case-sensitive substring of its RAW bytes (the Rust
//              tokenizer cuts those out before it normalises), anywhere in the row: status 1, length 0, id row zero.  The caller encodes such a row itself.
//
// One set of __host__ __device__ primitives (class table, lower-casing, the "not ours" test of a byte position, the table probe, the greedy match of one word)
// under two drivers: wp_encode_text, the rule on the host, one byte at a time, and wp_encode_kernel, one wave per text.
//
// THE RULE FOR UTF-8 TEXT (mv_tok_encode_u8*; opt-in: an object serves it once mv_tok_set_unicode has given it a code-point table)
//   below 0x80 exactly the ASCII rule above (wp_class, wp_lower); the code-point table is never read for such a byte, so an ASCII row's ids are the ASCII path's.
//   U+0080 .. U+1FFFF, as a well-formed UTF-8 sequence, is replaced by its table entry (WpCp): the UTF-8 bytes of the tokenizer's own
//              normalizer.normalize_str(chr(cp)) — 0 to 3 code points, at most 12 bytes; clean, the CJK spacing, accent stripping and lower-casing are already in
//              it — and one class per OUTPUT code point (word, punctuation, whitespace), as the tokenizer's own pre-tokenizer treats that character.
//   split      on the classes of the output characters; a punctuation character is a word of its own.
//   WordPiece  per word the longest vocabulary entry from the left; prefixes end at character boundaries (a prefix that ends inside a character cannot equal
//              a valid-UTF-8 entry: skipping those probes is only an economy); max_chars counts CHARACTERS, for words and for vocabulary entries alike.
//   specials   and truncation as above.
//   not ours   status 2 (length 0, id row zero, like status 1): a row that holds a malformed sequence (stray continuation byte, truncated sequence, overlong
//              form, surrogate ED A0..BF, lead bytes F5..FF and so the 5- and 6-byte forms), a code point >= U+20000, or a code point the table marks uncovered
//              (decided where the table is made: memvul_amd/tokenizer.py).  The added-token literal rule stays, on the raw bytes: status 1, and status 1 wins
//              when both apply.
// Its drivers: wp_encode_text_u8, the rule on the host, one code point at a time (the rule's reference), and wp_encode_u8_kernel, one wave per text.
//
// The vocabulary table: open addressing (linear probing) over a power-of-two number of 16-byte slots, at least twice the entries (load <= 0.5); the key is
// FNV-1a of the piece's bytes, seeded by the continuation flag; EVERY hit is confirmed by comparing the bytes with the pooled copy of the vocabulary string, so
// the result never depends on two hashes being different.  Empty entries and ones of more than max_chars characters are left out: no word that reaches the
// matcher can equal them.  Entries with a byte >= 0x80 are in the table for the UTF-8 rule; an ASCII word cannot equal one, and max_len0 / max_len1, the bounds
// of the ASCII matcher's search, are taken over the ASCII entries alone (WpHost::max_len0_all / max_len1_all: over all of them, in bytes).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define WP_HD __host__ __device__ __forceinline__
#else
#define WP_HD inline
#endif

#define WP_MAX_CHARS_LIMIT 190  // the kernel's word buffer: a carried word (<= max_chars bytes) plus one 64-byte step fit 256 bytes
#define WP_MAX_LENGTH 512

struct alignas(16) WpSlot {
  uint32_t hash;
  uint32_t off;  // of the entry's bytes in the pool
  uint32_t key;  // length | continuation << 16; 0 = empty slot
  int32_t id;
};

struct WpTable {  // plain pointers: the host's copy points into WpHost, the device's into device memory
  const WpSlot* slots;
  const uint8_t* pool;
  const uint8_t* lit;       // the added-token literals back to back
  const uint32_t* lit_off;  // [n_lit + 1]
  uint64_t lit_first0, lit_first1;  // bit b of the pair: some literal starts with byte b (scalars, not an array: no dynamic index into a kernel argument)
  uint32_t mask;            // slots - 1
  int32_t n_lit;
  int32_t max_len0, max_len1;  // longest entry among first pieces / continuations: bounds the greedy search
  int32_t unk, cls, sep, max_chars, lowercase;
};

// ---- UTF-8: the code-point table and what the UTF-8 drivers need beside WpTable (a second kernel argument: WpTable's layout is wp_encode_kernel's) ------------
#define WP_U8_CODE_POINTS 0x20000  // entry i is code point i; entries below 0x80 are never read
#define WP_U8_BUF 640              // the kernel's word buffer, bytes: a carried word (<= max_chars characters of <= 4 bytes) plus one step's largest output fit
#define WP_U8_STARTS 256           // its start list: one step's largest output + 1 (the carried word) fit

struct alignas(16) WpCp {
  uint8_t out[12];  // UTF-8 of normalize_str(chr(cp))
  uint8_t nbytes;   // 0 .. 12
  uint8_t cls;      // two bits per output code point, the first in the low bits: 1 whitespace, 2 punctuation, 3 word (wp_class's codes)
  uint8_t covered;  // 0: a row that holds this code point is handed back (status 2)
  uint8_t nchars;   // 0 .. 3 output code points
};

struct WpU8 {
  const WpCp* cp;
  int32_t n_cp;                // code points >= n_cp are uncovered
  int32_t max_len0, max_len1;  // longest entry, in bytes, among ALL first pieces / continuations
  uint64_t lit_first2, lit_first3;  // WpTable::lit_first0 / 1 continued: bit b of the pair: some literal starts with byte 128 + b
};

// ---- the 128-entry class table, two bits per byte: 0 removed, 1 whitespace, 2 punctuation, 3 word byte ----------------------------------------------------------
constexpr int wp_class_of(int c) {
  return (c == 9 || c == 10 || c == 13 || c == 32) ? 1
         : (c < 32 || c == 127)                    ? 0
         : ((c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126)) ? 2 : 3;
}
constexpr uint64_t wp_class_word(int w) {
  uint64_t v = 0;
  for (int i = 0; i < 32; ++i) v |= (uint64_t)wp_class_of(w * 32 + i) << (2 * i);
  return v;
}
WP_HD int wp_class(uint32_t c) {  // c < 128
  constexpr uint64_t k0 = wp_class_word(0), k1 = wp_class_word(1), k2 = wp_class_word(2), k3 = wp_class_word(3);
  const uint64_t w = c < 64 ? (c < 32 ? k0 : k1) : (c < 96 ? k2 : k3);
  return (int)((w >> ((c & 31) * 2)) & 3);
}
WP_HD uint32_t wp_lower(uint32_t c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

WP_HD uint32_t wp_hash_seed(int cont) { return cont ? 0x9747b28cu : 0x811c9dc5u; }
WP_HD uint32_t wp_hash_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }
WP_HD uint32_t wp_home(uint32_t h) { return h ^ (h >> 16); }

// one of the added-token literals starts at p (`left` = bytes from p to the end of the row, >= 1): the comparison, behind the callers' first-byte filters
WP_HD bool wp_literal_starts(const WpTable& t, const uint8_t* p, int64_t left) {
  for (int k = 0; k < t.n_lit; ++k) {
    const uint8_t* l = t.lit + t.lit_off[k];
    const int64_t n = (int64_t)t.lit_off[k + 1] - t.lit_off[k];
    if (n > left) continue;
    int64_t j = 0;
    while (j < n && l[j] == p[j]) ++j;
    if (j == n) return true;
  }
  return false;
}

// "not ours", tested at one byte position: p[0] >= 0x80, or an added-token literal starts at p
WP_HD bool wp_foreign_at(const WpTable& t, const uint8_t* p, int64_t left) {
  const uint32_t c = p[0];
  if (c >= 0x80) return true;
  if (!(((c < 64 ? t.lit_first0 : t.lit_first1) >> (c & 63)) & 1)) return false;
  return wp_literal_starts(t, p, left);
}

// the id of the entry with exactly the bytes w[0, len) and the flag `cont` (h = their hash), or -1
template <typename BytePtr>
WP_HD int32_t wp_lookup(const WpTable& t, uint32_t h, BytePtr w, int len, int cont) {
  const uint32_t key = (uint32_t)len | ((uint32_t)cont << 16);
  for (uint32_t i = wp_home(h) & t.mask;; i = (i + 1) & t.mask) {  // ends: at most half the slots are taken
    const WpSlot s = t.slots[i];
    if (s.key == 0) return -1;
    if (s.hash == h && s.key == key) {
      const uint8_t* p = t.pool + s.off;
      int j = 0;
      while (j < len && p[j] == w[j]) ++j;
      if (j == len) return s.id;
    }
  }
}

// One word w[0, len), 1 <= len <= max_chars, already cleaned and lower-cased: piece[p] = the id of the piece that starts at byte p.  `piece` [len] holds -1 on
// entry.  A word with an unmatched remainder leaves piece[0] = [UNK] and nothing else.
template <typename BytePtr, typename IdPtr>
WP_HD void wp_match_word(const WpTable& t, BytePtr w, int len, IdPtr piece) {
  int p = 0;
  while (p < len) {
    const int cont = p > 0 ? 1 : 0;
    const int longest = cont ? t.max_len1 : t.max_len0;
    const int lim = len - p < longest ? len - p : longest;
    uint32_t h = wp_hash_seed(cont);
    int32_t best = -1;
    int best_len = 0;
    for (int q = 0; q < lim; ++q) {  // every prefix, shortest first: the hash grows a byte at a time, the longest hit stays
      h = wp_hash_step(h, w[p + q]);
      const int32_t id = wp_lookup(t, h, w + p, q + 1, cont);
      if (id >= 0) { best = id; best_len = q + 1; }
    }
    if (best < 0) {
      for (int j = 1; j < p; ++j) piece[j] = -1;
      piece[0] = t.unk;
      return;
    }
    piece[p] = best;
    p += best_len;
  }
}

// ---- UTF-8 primitives ------------------------------------------------------------------------------------------------------------------------------------------------
// an added-token literal starts at p, whatever its bytes: the UTF-8 rule's test of a byte position.  A literal may hold bytes >= 0x80 (an emoji or an arrow given to
// add_special_tokens): the Rust tokenizer cuts it out of the raw text like any other, so it is matched on the raw bytes like any other; the first-byte filter
// for bytes >= 0x80 travels in WpU8.
WP_HD bool wp_literal_at(const WpTable& t, const WpU8& u, const uint8_t* p, int64_t left) {
  const uint32_t c = p[0];
  const uint64_t first = c < 64 ? t.lit_first0 : c < 128 ? t.lit_first1 : c < 192 ? u.lit_first2 : u.lit_first3;
  return ((first >> (c & 63)) & 1) && wp_literal_starts(t, p, left);
}

// The sequence that starts at p (`left` >= 1 bytes to the end of the row): its length 1 .. 4 and its code point, or 0 when it is malformed — p[0] a continuation
// byte, C0 / C1 / F5 .. FF, a sequence cut by the end of the row, a byte that is no continuation where one is due, an overlong form (E0 80..9F, F0 80..8F), a
// surrogate (ED A0..BF) or a code point past U+10FFFF (F4 90..).
WP_HD int wp_u8_decode(const uint8_t* p, int64_t left, uint32_t* cp) {
  const uint32_t b0 = p[0];
  if (b0 < 0x80) { *cp = b0; return 1; }
  if (b0 < 0xC2 || b0 > 0xF4) return 0;
  const int len = b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
  if (left < len) return 0;
  const uint32_t b1 = p[1];
  const uint32_t lo = b0 == 0xE0 ? 0xA0u : b0 == 0xF0 ? 0x90u : 0x80u, hi = b0 == 0xED ? 0x9Fu : b0 == 0xF4 ? 0x8Fu : 0xBFu;
  if (b1 < lo || b1 > hi) return 0;
  uint32_t c = ((b0 & (0xFFu >> (len + 1))) << 6) | (b1 & 0x3F);
  for (int j = 2; j < len; ++j) {
    const uint32_t b = p[j];
    if ((b & 0xC0) != 0x80) return 0;
    c = (c << 6) | (b & 0x3F);
  }
  *cp = c;
  return len;
}

// p[0] is a continuation byte: does a lead byte at most three bytes back, not before `row`, reach it?  (Whether that sequence is well formed is the lead
// byte's test.)  The kernel's lanes decide "stray continuation byte" with it; the host decodes sequence by sequence and meets a stray one as a first byte.
WP_HD bool wp_u8_cont_reached(const uint8_t* row, const uint8_t* p) {
  for (int d = 1; d <= 3 && p - d >= row; ++d) {
    const uint32_t b = p[-d];
    if ((b & 0xC0) == 0x80) continue;
    return (b < 0xC0 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4) > d;
  }
  return false;
}

// wp_match_word for a word of whole UTF-8 characters, len <= 4 * max_chars bytes: the same greedy search, probing only prefixes that end at a character boundary;
// longest0 / longest1: WpU8::max_len0 / max_len1.
template <typename BytePtr, typename IdPtr>
WP_HD void wp_match_word_u8(const WpTable& t, int longest0, int longest1, BytePtr w, int len, IdPtr piece) {
  int p = 0;
  while (p < len) {
    const int cont = p > 0 ? 1 : 0;
    const int longest = cont ? longest1 : longest0;
    const int lim = len - p < longest ? len - p : longest;
    uint32_t h = wp_hash_seed(cont);
    int32_t best = -1;
    int best_len = 0;
    for (int q = 0; q < lim; ++q) {
      h = wp_hash_step(h, w[p + q]);
      if (p + q + 1 < len && (w[p + q + 1] & 0xC0) == 0x80) continue;  // inside a character
      const int32_t id = wp_lookup(t, h, w + p, q + 1, cont);
      if (id >= 0) { best = id; best_len = q + 1; }
    }
    if (best < 0) {
      for (int j = 1; j < p; ++j) piece[j] = -1;
      piece[0] = t.unk;
      return;
    }
    piece[p] = best;
    p += best_len;
  }
}

// ---- the table, built on the host ---------------------------------------------------------------------------------------------------------------------------------
struct WpHost {
  std::vector<WpSlot> slots;
  std::vector<uint8_t> pool, lit;
  std::vector<uint32_t> lit_off;
  WpTable t;
  int32_t max_len0_all = 0, max_len1_all = 0;  // WpU8::max_len0 / max_len1
  uint64_t lit_first2 = 0, lit_first3 = 0;     // WpU8::lit_first2 / lit_first3
};

// entry k of the vocabulary (bytes vocab_off[k] .. vocab_off[k + 1]) has id k; "##x" is the continuation x.  false + err on a bad argument.
inline bool wp_build(WpHost& H, const char* vocab_bytes, const int64_t* vocab_off, int n_vocab, const char* literal_bytes, const int64_t* literal_off,
                     int n_literals, int unk, int cls, int sep, int max_chars, int lowercase, std::string& err) {
  if (n_vocab <= 0 || !vocab_off || n_literals < 0 || (n_literals > 0 && !literal_off)) { err = "mv_tok_create: NULL or empty vocabulary / literal list"; return false; }
  if (max_chars < 1 || max_chars > WP_MAX_CHARS_LIMIT) { err = "mv_tok_create: max_chars_per_word outside 1 .. " + std::to_string(WP_MAX_CHARS_LIMIT); return false; }
  if (unk < 0 || unk >= n_vocab || cls < 0 || cls >= n_vocab || sep < 0 || sep >= n_vocab) { err = "mv_tok_create: a special id outside the vocabulary"; return false; }
  for (int k = 0; k < n_vocab; ++k)
    if (vocab_off[k] < 0 || vocab_off[k + 1] < vocab_off[k]) { err = "mv_tok_create: vocabulary offsets not ascending"; return false; }
  for (int k = 0; k < n_literals; ++k)
    if (literal_off[k] < 0 || literal_off[k + 1] <= literal_off[k]) { err = "mv_tok_create: literal offsets not ascending (an empty literal matches everywhere)"; return false; }
  if ((vocab_off[n_vocab] > vocab_off[0] && !vocab_bytes) || (n_literals > 0 && !literal_bytes)) { err = "mv_tok_create: NULL bytes"; return false; }
  if (vocab_off[n_vocab] - vocab_off[0] > 0x7fffffff) { err = "mv_tok_create: vocabulary larger than 2 GiB"; return false; }
  size_t cap = 16;
  while (cap < 2 * (size_t)n_vocab) cap <<= 1;
  H.slots.assign(cap, WpSlot{0, 0, 0, 0});
  H.pool.clear();
  H.pool.reserve((size_t)(vocab_off[n_vocab] - vocab_off[0]) + 1);
  WpTable& t = H.t;
  t.mask = (uint32_t)cap - 1;
  t.max_len0 = t.max_len1 = 0;
  H.max_len0_all = H.max_len1_all = 0;
  t.unk = unk; t.cls = cls; t.sep = sep; t.max_chars = max_chars; t.lowercase = lowercase ? 1 : 0;
  for (int k = 0; k < n_vocab; ++k) {
    const uint8_t* s = (const uint8_t*)vocab_bytes + vocab_off[k];
    int64_t n = vocab_off[k + 1] - vocab_off[k];
    int cont = 0;
    if (n > 2 && s[0] == '#' && s[1] == '#') { cont = 1; s += 2; n -= 2; }
    if (n < 1 || n > 4 * (int64_t)max_chars) continue;  // (more bytes than max_chars characters can have)
    bool ascii = true;
    int chars = 0;
    uint32_t h = wp_hash_seed(cont);
    for (int64_t j = 0; j < n; ++j) { ascii &= s[j] < 0x80; chars += (s[j] & 0xC0) != 0x80; h = wp_hash_step(h, s[j]); }
    if (chars > max_chars) continue;
    const uint32_t key = (uint32_t)n | ((uint32_t)cont << 16);
    uint32_t i = wp_home(h) & t.mask;
    for (;; i = (i + 1) & t.mask) {
      WpSlot& sl = H.slots[i];
      if (sl.key == 0) {
        sl = WpSlot{h, (uint32_t)H.pool.size(), key, k};
        H.pool.insert(H.pool.end(), s, s + n);
        break;
      }
      if (sl.hash == h && sl.key == key && std::memcmp(H.pool.data() + sl.off, s, (size_t)n) == 0) { sl.id = k; break; }  // the same string again: the later id, as a dict built in order keeps
    }
    int32_t& longest_all = cont ? H.max_len1_all : H.max_len0_all;
    if ((int)n > longest_all) longest_all = (int)n;
    if (!ascii) continue;
    int32_t& longest = cont ? t.max_len1 : t.max_len0;
    if ((int)n > longest) longest = (int)n;
  }
  if (H.pool.empty()) H.pool.push_back(0);
  H.lit.clear();
  H.lit_off.assign(1, 0u);
  t.lit_first0 = t.lit_first1 = H.lit_first2 = H.lit_first3 = 0;
  for (int k = 0; k < n_literals; ++k) {  // every literal, also one with bytes >= 0x80: the ASCII rule hands a row that could hold such a one back for those bytes
    const uint8_t* s = (const uint8_t*)literal_bytes + literal_off[k];  // anyway and never compares it (no ASCII row matches it), the UTF-8 rule needs it
    const int64_t n = literal_off[k + 1] - literal_off[k];
    H.lit.insert(H.lit.end(), s, s + n);
    H.lit_off.push_back((uint32_t)H.lit.size());
    (s[0] < 64 ? t.lit_first0 : s[0] < 128 ? t.lit_first1 : s[0] < 192 ? H.lit_first2 : H.lit_first3) |= 1ull << (s[0] & 63);
  }
  t.n_lit = (int32_t)H.lit_off.size() - 1;
  if (H.lit.empty()) H.lit.push_back(0);
  t.slots = H.slots.data(); t.pool = H.pool.data(); t.lit = H.lit.data(); t.lit_off = H.lit_off.data();
  return true;
}

// ---- the rule on the host: one text, one byte at a time -------------------------------------------------------------------------------------------------------------
inline void wp_encode_text(const WpTable& t, const uint8_t* s, int64_t n, int max_length, int add_special, int32_t* ids, int32_t* len, uint8_t* status) {
  for (int i = 0; i < max_length; ++i) ids[i] = 0;
  for (int64_t i = 0; i < n; ++i)
    if (wp_foreign_at(t, s + i, n - i)) { *len = 0; *status = 1; return; }
  const int budget = max_length - (add_special ? 2 : 0), base = add_special ? 1 : 0;
  int32_t* out = ids + base;
  int nout = 0, wl = 0;  // wl: bytes of the word in progress, counted past the buffer's end
  uint8_t word[WP_MAX_CHARS_LIMIT];
  int32_t piece[WP_MAX_CHARS_LIMIT];
  auto flush = [&]() {
    if (wl == 0) return;
    if (wl > t.max_chars) {
      if (nout < budget) out[nout++] = t.unk;
    } else {
      for (int j = 0; j < wl; ++j) piece[j] = -1;
      wp_match_word(t, (const uint8_t*)word, wl, piece);
      for (int j = 0; j < wl && nout < budget; ++j)
        if (piece[j] >= 0) out[nout++] = piece[j];
    }
    wl = 0;
  };
  for (int64_t i = 0; i < n && nout < budget; ++i) {
    const uint32_t c = s[i];
    const int k = wp_class(c);
    if (k == 0) continue;
    if (k == 3) {
      if (wl < t.max_chars) word[wl] = (uint8_t)(t.lowercase ? wp_lower(c) : c);
      if (wl <= t.max_chars) ++wl;
      continue;
    }
    flush();
    if (k == 2 && nout < budget) { wl = 1; word[0] = (uint8_t)c; flush(); }
  }
  if (nout < budget) flush();
  if (add_special) { ids[0] = t.cls; ids[base + nout] = t.sep; }
  *len = base + nout + (add_special ? 1 : 0);
  *status = 0;
}

// ---- the code-point table, checked on the host --------------------------------------------------------------------------------------------------------------------
// What mv_tok_set_unicode refuses: an entry (from 0x80 on) with more than 12 bytes or 3 characters, output bytes that are not well-formed UTF-8, a character
// count that is not the bytes', a class outside the three; and a table whose largest output per 64-byte step does not fit the kernel's buffers beside a carried
// word of max_chars characters.  A step's lanes hold the first bytes of sequences that together lie in 64 + 3 bytes of input (the last may straddle the step's
// end), so its output is at most 67 x the table's largest ratio of output bytes to input bytes (never below 1: an ASCII byte gives one byte).
inline bool wp_u8_check_table(const WpCp* e, int n, int max_chars, std::string& err) {
  if (!e || n < 1 || n > WP_U8_CODE_POINTS) { err = "mv_tok_set_unicode: NULL table or n_entries outside 1 .. 131072"; return false; }
  int num = 1, den = 1;  // the largest output / input byte ratio
  for (int i = 0x80; i < n; ++i) {
    const WpCp& c = e[i];
    const std::string at = "mv_tok_set_unicode: entry " + std::to_string(i);
    if (c.nbytes > 12 || c.nchars > 3 || c.covered > 1) { err = at + ": byte count over 12, more than 3 characters or a covered flag that is neither 0 nor 1"; return false; }
    int chars = 0;
    for (int j = 0; j < c.nbytes;) {
      uint32_t cp;
      const int len = wp_u8_decode(c.out + j, c.nbytes - j, &cp);
      if (len == 0) { err = at + ": output bytes are not well-formed UTF-8"; return false; }
      if (chars >= 3 || ((c.cls >> (2 * chars)) & 3) == 0) { err = at + ": a class outside whitespace / punctuation / word, or more than 3 characters"; return false; }
      ++chars;
      j += len;
    }
    if (chars != c.nchars) { err = at + ": the character count is not that of the output bytes"; return false; }
    const int in = i < 0x800 ? 2 : i < 0x10000 ? 3 : 4;
    if (c.covered && c.nbytes * den > num * in) { num = c.nbytes; den = in; }
  }
  const int step = 67 * num / den;
  if (4 * max_chars + step > WP_U8_BUF || step + 1 > WP_U8_STARTS) {
    err = "mv_tok_set_unicode: a carried word of max_chars_per_word = " + std::to_string(max_chars) + " characters and one step's largest output (" + std::to_string(step) +
          " bytes) do not fit the kernel's " + std::to_string(WP_U8_BUF) + "-byte word buffer";
    return false;
  }
  return true;
}

// ---- the UTF-8 rule on the host: one text, one code point at a time ----------------------------------------------------------------------------------------------
inline void wp_encode_text_u8(const WpTable& t, const WpU8& u, const uint8_t* s, int64_t n, int max_length, int add_special, int32_t* ids, int32_t* len,
                              uint8_t* status) {
  for (int i = 0; i < max_length; ++i) ids[i] = 0;
  *len = 0;
  for (int64_t i = 0; i < n; ++i)
    if (wp_literal_at(t, u, s + i, n - i)) { *status = 1; return; }
  for (int64_t i = 0; i < n;) {
    uint32_t cp;
    const int l = wp_u8_decode(s + i, n - i, &cp);
    if (l == 0 || (cp >= 0x80 && (cp >= (uint32_t)u.n_cp || !u.cp[cp].covered))) { *status = 2; return; }
    i += l;
  }
  const int budget = max_length - (add_special ? 2 : 0), base = add_special ? 1 : 0;
  int32_t* out = ids + base;
  int nout = 0, wl = 0, wc = 0;  // bytes and characters of the word in progress; the characters are counted one past max_chars
  uint8_t word[4 * WP_MAX_CHARS_LIMIT];
  int32_t piece[4 * WP_MAX_CHARS_LIMIT];
  auto flush = [&]() {
    if (wc == 0) return;
    if (wc > t.max_chars) {
      if (nout < budget) out[nout++] = t.unk;
    } else {
      for (int j = 0; j < wl; ++j) piece[j] = -1;
      wp_match_word_u8(t, u.max_len0, u.max_len1, (const uint8_t*)word, wl, piece);
      for (int j = 0; j < wl && nout < budget; ++j)
        if (piece[j] >= 0) out[nout++] = piece[j];
    }
    wl = wc = 0;
  };
  auto put = [&](const uint8_t* b, int nb, int k) {  // one output character of class k
    if (k == 3) {
      if (wc < t.max_chars) { std::memcpy(word + wl, b, (size_t)nb); wl += nb; }
      if (wc <= t.max_chars) ++wc;
      return;
    }
    flush();
    if (k == 2 && nout < budget) { std::memcpy(word, b, (size_t)nb); wl = nb; wc = 1; flush(); }
  };
  for (int64_t i = 0; i < n && nout < budget;) {
    uint32_t cp;
    i += wp_u8_decode(s + i, n - i, &cp);
    if (cp < 0x80) {
      const int k = wp_class(cp);
      const uint8_t b = (uint8_t)(t.lowercase ? wp_lower(cp) : cp);
      if (k != 0) put(&b, 1, k);
      continue;
    }
    const WpCp& e = u.cp[cp];
    for (int j = 0, ch = 0; j < e.nbytes && nout < budget; ++ch) {
      const int l = e.out[j] < 0x80 ? 1 : e.out[j] < 0xE0 ? 2 : e.out[j] < 0xF0 ? 3 : 4;
      put(e.out + j, l, (e.cls >> (2 * ch)) & 3);
      j += l;
    }
  }
  if (nout < budget) flush();
  if (add_special) { ids[0] = t.cls; ids[base + nout] = t.sep; }
  *len = base + nout + (add_special ? 1 : 0);
  *status = 0;
}

#ifdef __HIPCC__
// ---- the kernel: one wave per text, four waves per workgroup, no barrier between the waves (texts differ in length) -----------------------------------------------
// Per 64-byte step, one byte per lane (the position one past the text's end reads as a space, so the last word always ends):
//   1. the "not ours" test of the lane's position on the raw bytes (a literal's tail is read from global memory, so it may cross steps); a hit ends the row;
//   2. class and lower-casing, then the kept bytes — everything but the removed class, whitespace as ' ' — are compacted behind the carried word in the wave's
//      word buffer (ballot + popcount prefix): cleaning comes before splitting, because a removed byte joins its neighbours;
//   3. word starts of the new bytes from the classes in the buffer, compacted into a start list (the carried word is entry 0);
//   4. a lane per word: its end, then wp_match_word into piece[] (indexed by the byte a piece starts at, so buffer order is token order); the word that
//      touches the buffer's end is not matched: it moves to the front and carries over — or, past max_chars bytes, shrinks to a one-byte stand-in that
//      becomes [UNK] when it ends;
//   5. the pieces of the finished words are compacted to the output row (ballot + popcount prefix again) up to the token budget; a full budget ends the
//      tokenising, the "not ours" scan goes on to the end of the row.
// LDS per wave: the word buffer is 256 bytes = 64 dwords.  Byte reads and every write bank as (address / 4) % 32 within a 32-lane half, so dwords d and d + 32 of
// the buffer share a bank: two lanes of one half whose words lie 128 bytes apart can meet, at most 2-way (lanes in one dword share a broadcast); piece[] is
// 256 dwords, a write meets only a piece start a multiple of 32 dwords away.  Neither is measured (SQ_LDS_BANK_CONFLICT): the table probes in global memory
// dominate a step.  5.5 KB per workgroup.  No atomics, no inline assembly, no scratch.
__device__ __forceinline__ void wp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

#ifndef WP_U8_KERNEL  // (wordpiece_u8.hip defines it: that file compiles the UTF-8 kernel, every other the ASCII one)
__global__ __launch_bounds__(256) void wp_encode_kernel(const WpTable t, const uint8_t* __restrict__ text, const int64_t* __restrict__ off, int n, int max_length,
                                                        int add_special, int32_t* __restrict__ ids, int32_t* __restrict__ lens, uint8_t* __restrict__ status) {
  __shared__ uint8_t s_buf[4][256];
  __shared__ int32_t s_piece[4][256];
  __shared__ uint8_t s_start[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  if (row >= n) return;  // the whole wave
  uint8_t* buf = s_buf[wv];
  int32_t* piece = s_piece[wv];
  uint8_t* start = s_start[wv];
  const uint64_t below = (1ull << lane) - 1;
  const int64_t t0 = off[row], t1 = off[row + 1];
  int32_t* out = ids + row * max_length;
  const int budget = max_length - (add_special ? 2 : 0), base = add_special ? 1 : 0;
  int nout = 0, fill = 0;  // fill: bytes of the carried word at the front of the buffer (<= max_chars)
  bool overlong = false;   // the carried word has passed max_chars bytes: buf[0] stands for it
  bool foreign = false, full = budget <= 0;
  for (int64_t p = t0; p <= t1; p += 64) {
    const int64_t q = p + lane;
    const bool in = q < t1;
    const uint32_t c = in ? text[q] : 32u;
    if (__ballot(in && wp_foreign_at(t, text + q, t1 - q)) != 0) { foreign = true; break; }
    if (full) continue;
    const int k = wp_class(c & 127);
    if (fill == 0 && __ballot(k >= 2) == 0) continue;  // nothing but whitespace and removed bytes, no word in progress
    const uint64_t keep = __ballot(k != 0);
    if (k != 0) buf[fill + __popcll(keep & below)] = (uint8_t)(k == 1 ? 32u : (t.lowercase ? wp_lower(c) : c));
    const int nk = __popcll(keep), nf = fill + nk;  // nf <= max_chars + 64 <= 254
    for (int i = lane; i < nf; i += 64) piece[i] = -1;
    wp_wave_sync();
    bool is_start = false;
    if (lane < nk) {
      const int pos = fill + lane, kc = wp_class(buf[pos]);
      is_start = kc == 2 || (kc == 3 && (pos == 0 || wp_class(buf[pos - 1]) != 3));
    }
    const uint64_t sm = __ballot(is_start);
    const int carry = fill > 0 ? 1 : 0, nw = carry + __popcll(sm);
    if (carry && lane == 0) start[0] = 0;
    if (is_start) start[carry + __popcll(sm & below)] = (uint8_t)(fill + lane);
    wp_wave_sync();
    int tail = -1;  // where the unfinished last word starts
    for (int w0 = 0; w0 < nw; w0 += 64) {
      const int w = w0 + lane;
      bool unfinished = false;
      int s = 0;
      if (w < nw) {
        s = start[w];
        int e = s + 1;
        const bool punct = wp_class(buf[s]) == 2;
        if (!punct)
          while (e < nf && wp_class(buf[e]) == 3) ++e;
        if (punct || e < nf) {
          if ((w == 0 && carry && overlong) || e - s > t.max_chars) piece[s] = t.unk;
          else wp_match_word(t, buf + s, e - s, piece + s);
        } else {
          unfinished = true;
        }
      }
      const uint64_t um = __ballot(unfinished);
      if (um != 0) tail = __shfl(s, __ffsll((long long)um) - 1);
    }
    wp_wave_sync();
    const int limit = tail >= 0 ? tail : nf;
    for (int i0 = 0; i0 < limit && nout < budget; i0 += 64) {
      const int i = i0 + lane;
      const int32_t v = i < limit ? piece[i] : -1;
      const uint64_t m = __ballot(v >= 0);
      const int o = nout + __popcll(m & below);
      if (v >= 0 && o < budget) out[base + o] = v;
      nout += __popcll(m);
    }
    if (nout >= budget) { nout = budget; full = true; continue; }
    if (tail < 0) {
      fill = 0;
      overlong = false;
    } else if ((overlong && tail == 0) || nf - tail > t.max_chars) {
      overlong = true;
      fill = 1;
      if (lane == 0) buf[0] = 'a';
    } else {
      const int len = nf - tail;
      overlong = false;
      if (tail > 0)
        for (int i0 = 0; i0 < len; i0 += 64) {  // down to the front, 64 bytes at a time: a round's writes end below every later round's reads
          const int i = i0 + lane;
          const uint8_t b = i < len ? buf[tail + i] : 0;
          wp_wave_sync();
          if (i < len) buf[i] = b;
          wp_wave_sync();
        }
      fill = len;
    }
    wp_wave_sync();
  }
  if (foreign) {
    for (int i = lane; i < max_length; i += 64) out[i] = 0;
    if (lane == 0) { lens[row] = 0; status[row] = 1; }
    return;
  }
  const int total = base + nout + (add_special ? 1 : 0);
  if (lane == 0) {
    if (add_special) { out[0] = t.cls; out[base + nout] = t.sep; }
    lens[row] = total;
    status[row] = 0;
  }
  for (int i = total + lane; i < max_length; i += 64) out[i] = 0;
}
#else  // WP_U8_KERNEL
// Compiled by wordpiece_u8.hip alone, into a code object of its own (libmemvul_tok_u8.so): the kernels of libmemvul_hip.so, which the recorded bits of an encoder
// pass are keyed on, are the same set with or without the UTF-8 mode.
// ---- the UTF-8 kernel: one wave per text, four waves per workgroup, wp_encode_kernel's five stages with these differences ---------------------------------------------
//   1. the literal test alone ends the row (status 1); a malformed sequence, a code point >= n_cp or an uncovered one only stops the tokenising (status 2 unless
//      a literal follows: status 1 wins), so every step is decoded, also behind a full token budget;
//   2. one raw byte per lane; an ASCII lane emits its byte as in wp_encode_kernel; a lead-byte lane decodes its sequence — its continuation bytes come from
//      global memory, so a sequence may straddle a step — and reads ONE 16-byte table entry; a continuation lane emits nothing (it only checks that a lead
//      byte reaches it).  The outputs, 0 .. 12 bytes a lane, go behind the carried word at a wave-wide exclusive prefix sum of the byte counts (six shuffles),
//      with a class byte beside every byte: the character's class, + 4 on the bytes after its first;
//   3. word starts from the class bytes; positions are 16 bits wide;
//   4. the greedy match probes at character boundaries and the length test counts characters (class bytes below 4);
//   5. as before.  The carried word is at most max_chars characters = 4 * max_chars bytes, one step adds at most 67 x the table's largest output / input ratio
//      (wp_u8_check_table refuses a table or a max_chars that does not fit WP_U8_BUF / WP_U8_STARTS; the kernel tests the two bounds again before it writes).
// LDS per wave: 640 bytes + 640 class bytes + 640 piece ids + 256 starts of 16 bits = 4352 bytes, 17 KB per workgroup: nine workgroups fit the 160 KB of a CU,
// more than the registers allow.  No atomics, no inline assembly, no scratch (the 12 output bytes are taken from three registers in an unrolled loop).
__global__ __launch_bounds__(256) void wp_encode_u8_kernel(const WpTable t, const WpU8 u, const uint8_t* __restrict__ text, const int64_t* __restrict__ off, int n,
                                                           int max_length, int add_special, int32_t* __restrict__ ids, int32_t* __restrict__ lens,
                                                           uint8_t* __restrict__ status) {
  __shared__ uint8_t s_buf[4][WP_U8_BUF];
  __shared__ uint8_t s_cls[4][WP_U8_BUF];
  __shared__ int32_t s_piece[4][WP_U8_BUF];
  __shared__ uint16_t s_start[4][WP_U8_STARTS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  if (row >= n) return;  // the whole wave
  uint8_t* buf = s_buf[wv];
  uint8_t* cls = s_cls[wv];
  int32_t* piece = s_piece[wv];
  uint16_t* start = s_start[wv];
  const uint64_t below = (1ull << lane) - 1;
  const int64_t t0 = off[row], t1 = off[row + 1];
  int32_t* out = ids + row * max_length;
  const int budget = max_length - (add_special ? 2 : 0), base = add_special ? 1 : 0;
  int nout = 0, fill = 0;  // fill: bytes of the carried word at the front of the buffer (<= 4 * max_chars)
  bool overlong = false;   // the carried word has passed max_chars characters: buf[0] stands for it
  bool literal = false, bad = false, full = budget <= 0;
  for (int64_t p = t0; p <= t1; p += 64) {
    const int64_t q = p + lane;
    const bool in = q < t1;
    const uint32_t c = in ? text[q] : 32u;
    if (__ballot(in && wp_literal_at(t, u, text + q, t1 - q)) != 0) { literal = true; break; }
    if (bad) continue;
    // the lane's output: nb bytes in o0 .. o2, the classes of its characters in kk
    int nb = 0;
    uint32_t o0 = 0, o1 = 0, o2 = 0, kk = 0;
    bool bad_here = false;
    if (c < 0x80) {
      kk = (uint32_t)wp_class(c);
      nb = kk != 0 ? 1 : 0;
      o0 = kk == 1 ? 32u : (t.lowercase ? wp_lower(c) : c);
    } else if ((c & 0xC0) == 0x80) {
      bad_here = !wp_u8_cont_reached(text + t0, text + q);
    } else {
      uint32_t cp = 0;
      const int l = wp_u8_decode(text + q, t1 - q, &cp);
      if (l == 0 || cp >= (uint32_t)u.n_cp) {
        bad_here = true;
      } else {
        const uint4 e = *reinterpret_cast<const uint4*>(u.cp + cp);
        bad_here = ((e.w >> 16) & 0xFF) == 0;
        nb = bad_here ? 0 : (int)(e.w & 0xFF);
        kk = (e.w >> 8) & 0xFF;
        o0 = e.x; o1 = e.y; o2 = e.z;
      }
    }
    if (__ballot(bad_here) != 0) { bad = true; continue; }
    if (full) continue;
    if (fill == 0 && __ballot(nb > 0 && (kk & 0x2A) != 0) == 0) continue;  // no character of class 2 or 3 (bit 1 of a class), no word in progress
    int incl = nb;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int nk = __shfl(incl, 63), nf = fill + nk;
    if (nf > WP_U8_BUF || nk >= WP_U8_STARTS) { bad = true; continue; }  // (what wp_u8_check_table rules out, tested where the writes are)
    {
      const int o = fill + incl - nb;
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < nb) {
          const uint32_t b = ((j < 4 ? o0 : j < 8 ? o1 : o2) >> ((j & 3) * 8)) & 0xFF;
          const bool first = (b & 0xC0) != 0x80;
          if (first && j > 0) kk >>= 2;
          buf[o + j] = (uint8_t)b;
          cls[o + j] = (uint8_t)((kk & 3) | (first ? 0 : 4));
        }
    }
    for (int i = lane; i < nf; i += 64) piece[i] = -1;
    wp_wave_sync();
    const int carry = fill > 0 ? 1 : 0;
    int nw = carry;
    if (carry && lane == 0) start[0] = 0;
    for (int i0 = 0; i0 < nk; i0 += 64) {
      const int pos = fill + i0 + lane;
      bool is_start = false;
      if (pos < nf) {
        const int kc = cls[pos];
        is_start = kc == 2 || (kc == 3 && (pos == 0 || (cls[pos - 1] & 3) != 3));
      }
      const uint64_t sm = __ballot(is_start);
      if (is_start) start[nw + __popcll(sm & below)] = (uint16_t)pos;
      nw += __popcll(sm);
    }
    wp_wave_sync();
    int tail = -1;  // where the unfinished last word starts
    for (int w0 = 0; w0 < nw; w0 += 64) {
      const int w = w0 + lane;
      bool unfinished = false;
      int s = 0;
      if (w < nw) {
        s = start[w];
        int e = s + 1, chars = 1;
        const bool punct = cls[s] == 2;
        if (punct) {
          while (e < nf && (cls[e] & 4)) ++e;
        } else {
          while (e < nf && (cls[e] & 3) == 3) { chars += (cls[e] & 4) ? 0 : 1; ++e; }
        }
        if (punct || e < nf) {
          if ((w == 0 && carry && overlong) || chars > t.max_chars) piece[s] = t.unk;
          else wp_match_word_u8(t, u.max_len0, u.max_len1, buf + s, e - s, piece + s);
        } else {
          unfinished = true;
        }
      }
      const uint64_t um = __ballot(unfinished);
      if (um != 0) tail = __shfl(s, __ffsll((long long)um) - 1);
    }
    wp_wave_sync();
    const int limit = tail >= 0 ? tail : nf;
    for (int i0 = 0; i0 < limit && nout < budget; i0 += 64) {
      const int i = i0 + lane;
      const int32_t v = i < limit ? piece[i] : -1;
      const uint64_t m = __ballot(v >= 0);
      const int o = nout + __popcll(m & below);
      if (v >= 0 && o < budget) out[base + o] = v;
      nout += __popcll(m);
    }
    if (nout >= budget) { nout = budget; full = true; continue; }
    if (tail < 0) {
      fill = 0;
      overlong = false;
    } else {
      const int len = nf - tail;
      int chars = 0;
      for (int i0 = 0; i0 < len; i0 += 64) chars += __popcll(__ballot(i0 + lane < len && !(cls[tail + i0 + lane] & 4)));
      if ((overlong && tail == 0) || chars > t.max_chars) {
        overlong = true;
        fill = 1;
        if (lane == 0) { buf[0] = 'a'; cls[0] = 3; }
      } else {
        overlong = false;
        if (tail > 0)
          for (int i0 = 0; i0 < len; i0 += 64) {  // down to the front, 64 bytes at a time: a round's writes end below every later round's reads
            const int i = i0 + lane;
            const uint8_t b = i < len ? buf[tail + i] : 0, k = i < len ? cls[tail + i] : 0;
            wp_wave_sync();
            if (i < len) { buf[i] = b; cls[i] = k; }
            wp_wave_sync();
          }
        fill = len;
      }
    }
    wp_wave_sync();
  }
  if (literal || bad) {
    for (int i = lane; i < max_length; i += 64) out[i] = 0;
    if (lane == 0) { lens[row] = 0; status[row] = literal ? 1 : 2; }
    return;
  }
  const int total = base + nout + (add_special ? 1 : 0);
  if (lane == 0) {
    if (add_special) { out[0] = t.cls; out[base + nout] = t.sep; }
    lens[row] = total;
    status[row] = 0;
  }
  for (int i = total + lane; i < max_length; i += 64) out[i] = 0;
}
#endif  // WP_U8_KERNEL
#endif  // __HIPCC__
