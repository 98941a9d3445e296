// The UTF-8 host core of memvul_amd/csrc/wordpiece.h under the sanitizers: a stand-alone program (its own main; nothing here is loaded into python or needs a GPU).
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I memvul_amd/csrc tools/wordpiece_utf8_host_check.cpp -o wordpiece_utf8_host_check
//   ./wordpiece_utf8_host_check       -> "wordpiece_utf8_host_check: OK (<rows> rows)" and exit status 0
// It builds the vocabulary table with non-ASCII pieces and a hand-made code-point table (accented Latin-1 letters to their base letter, a punctuation and a
// whitespace character, removed characters, CJK with spaces around it, Hangul syllables to their jamo, an emoji, uncovered code points), runs edge rows,
// malformed rows and 300 fuzz rows through wp_encode_text_u8 at several max_length values, and compares every row with a naive restatement over std::map and
// std::string that decodes on its own.  It also compares the two ways "malformed" is decided — sequence by sequence, as the host driver does, and byte position
// by byte position (wp_u8_decode at lead bytes, wp_u8_cont_reached at continuation bytes), as the kernel's lanes do — and the refusals of wp_u8_check_table.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "wordpiece.h"

namespace {

std::string utf8(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) { s += (char)(0xC0 | (c >> 6)); s += (char)(0x80 | (c & 63)); }
  else if (c < 0x10000) { s += (char)(0xE0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  else { s += (char)(0xF0 | (c >> 18)); s += (char)(0x80 | ((c >> 12) & 63)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  return s;
}

// the naive decoder: code points of a string, or false; written from the definition (the value's range decides whether a form is overlong)
bool decode_all(const std::string& s, std::vector<uint32_t>& out) {
  out.clear();
  for (size_t i = 0; i < s.size();) {
    const unsigned b = (unsigned char)s[i];
    int len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 0;
    if (!len || i + (size_t)len > s.size()) return false;
    uint32_t c = len == 1 ? b : b & (0x7Fu >> len);
    for (int j = 1; j < len; ++j) {
      const unsigned x = (unsigned char)s[i + (size_t)j];
      if ((x >> 6) != 2) return false;
      c = (c << 6) | (x & 63);
    }
    static const uint32_t least[5] = {0, 0, 0x80, 0x800, 0x10000};
    if (c < least[len] || c > 0x10FFFF || (c >= 0xD800 && c <= 0xDFFF)) return false;
    out.push_back(c);
    i += (size_t)len;
  }
  return true;
}

struct Out { std::string bytes; int cls; };

struct Naive {
  std::map<std::string, int> vocab;
  std::map<uint32_t, std::vector<Out>> table;  // covered code points >= 0x80
  std::vector<std::string> literals;
  int unk, cls, sep, max_chars;
  bool lowercase;

  static int chars(const std::string& w) {
    int n = 0;
    for (unsigned char c : w) n += (c >> 6) != 2;
    return n;
  }

  void word(const std::vector<std::string>& w, std::vector<int>& out) const {  // a word as a list of characters
    if ((int)w.size() > max_chars) { out.push_back(unk); return; }
    std::vector<int> pieces;
    size_t start = 0;
    while (start < w.size()) {
      size_t end = w.size();
      int id = -1;
      for (; end > start; --end) {
        std::string key = start ? "##" : "";
        for (size_t k = start; k < end; ++k) key += w[k];
        auto it = vocab.find(key);
        if (it != vocab.end() && chars(it->first.substr(start ? 2 : 0)) <= max_chars) { id = it->second; break; }
      }
      if (id < 0) { out.push_back(unk); return; }
      pieces.push_back(id);
      start = end;
    }
    out.insert(out.end(), pieces.begin(), pieces.end());
  }

  int encode(const std::string& s, int max_length, bool special, std::vector<int>& ids) const {  // the status; ids without padding
    ids.clear();
    for (const std::string& l : literals)
      if (s.find(l) != std::string::npos) return 1;
    std::vector<uint32_t> cps;
    if (!decode_all(s, cps)) return 2;
    std::vector<Out> chars_out;
    for (uint32_t c : cps) {
      if (c < 0x80) {
        const bool ws = c == 9 || c == 10 || c == 13 || c == 32;
        if (!ws && (c < 32 || c == 127)) continue;
        const bool punct = (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126);
        chars_out.push_back({std::string(1, (char)((lowercase && c >= 'A' && c <= 'Z') ? c + 32 : c)), ws ? 1 : punct ? 2 : 3});
      } else {
        auto it = table.find(c);
        if (it == table.end()) return 2;
        chars_out.insert(chars_out.end(), it->second.begin(), it->second.end());
      }
    }
    std::vector<int> toks;
    std::vector<std::string> w;
    for (const Out& o : chars_out) {
      if (o.cls == 3) { w.push_back(o.bytes); continue; }
      if (!w.empty()) word(w, toks);
      w.clear();
      if (o.cls == 2) word({o.bytes}, toks);
    }
    if (!w.empty()) word(w, toks);
    const size_t budget = (size_t)(max_length - (special ? 2 : 0));
    if (toks.size() > budget) toks.resize(budget);
    if (special) ids.push_back(cls);
    ids.insert(ids.end(), toks.begin(), toks.end());
    if (special) ids.push_back(sep);
    return 0;
  }
};

int fails = 0;

void compare(const WpTable& t, const WpU8& u, const Naive& nv, const std::string& s, int max_length, bool special) {
  std::vector<int32_t> ids((size_t)max_length, 12345);
  int32_t len = -7;
  uint8_t status = 9;
  wp_encode_text_u8(t, u, (const uint8_t*)s.data(), (int64_t)s.size(), max_length, special ? 1 : 0, ids.data(), &len, &status);
  std::vector<int> want;
  const int st = nv.encode(s, max_length, special, want);
  if (st != 0) want.clear();
  bool ok = status == st && len == (int32_t)want.size();
  for (int i = 0; ok && i < max_length; ++i) ok = ids[(size_t)i] == (i < (int)want.size() ? want[(size_t)i] : 0);
  if (!ok && fails++ < 5)
    std::fprintf(stderr, "MISMATCH max_length %d special %d len %d want %zu status %d want %d text[%zu] %.60s\n", max_length, (int)special, len, want.size(), status, st, s.size(), s.c_str());
}

// "malformed" as the kernel's lanes decide it, position by position, against the sequential decision
void compare_malformed(const std::string& s) {
  const uint8_t* p = (const uint8_t*)s.data();
  const int64_t n = (int64_t)s.size();
  bool by_position = false;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t cp;
    if (p[i] < 0x80) continue;
    if ((p[i] & 0xC0) == 0x80) by_position |= !wp_u8_cont_reached(p, p + i);
    else by_position |= wp_u8_decode(p + i, n - i, &cp) == 0;
  }
  std::vector<uint32_t> cps;
  if (by_position == decode_all(s, cps) && fails++ < 5) std::fprintf(stderr, "MALFORMED decided differently: text[%zu] %.60s\n", s.size(), s.c_str());
}

}  // namespace

int main() {
  std::vector<std::string> vocab = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"};
  for (char c = 'a'; c < 'z'; ++c) { vocab.push_back(std::string(1, c)); vocab.push_back(std::string("##") + c); }
  for (int c = 33; c < 126; ++c)
    if ((c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || c >= 123) vocab.push_back(std::string(1, (char)c));
  const std::string ss = utf8(0xDF), euro = utf8(0x20AC), zhong = utf8(0x4E2D), grin = utf8(0x1F600), g = utf8(0x1100), a = utf8(0x1161), dash = utf8(0x2014);
  for (const std::string& w : {std::string("ab"), std::string("abab"), std::string("cafe"), std::string("heap"), std::string("##ab"), ss, "##" + ss, euro, "##" + euro, zhong,
                               grin, "##" + grin, g, "##" + a, dash, "stra" + ss + "e", std::string(99, 'q') + ss, "##" + std::string(98, 'b') + ss,
                               std::string(100, 'q') + ss /* 101 characters: left out */, std::string("##"), std::string("\xa9\xa9") /* no UTF-8: never matched */, std::string()})
    vocab.push_back(w);
  std::string bytes, lit_bytes;
  std::vector<int64_t> off{0}, lit_off{0};
  Naive nv;
  for (size_t k = 0; k < vocab.size(); ++k) {
    bytes += vocab[k];
    off.push_back((int64_t)bytes.size());
    if (!vocab[k].empty()) nv.vocab[vocab[k]] = (int)k;
  }
  nv.literals = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", utf8(0x2192), "k" + utf8(0xE9)};  // two added tokens with bytes >= 0x80: matched on the raw bytes too
  for (const std::string& l : nv.literals) { lit_bytes += l; lit_off.push_back((int64_t)lit_bytes.size()); }
  nv.unk = 1; nv.cls = 2; nv.sep = 3; nv.max_chars = 100;

  // the code-point table, and the same content for the naive side
  std::vector<WpCp> cp(WP_U8_CODE_POINTS);
  std::memset(cp.data(), 0, cp.size() * sizeof(WpCp));
  auto set = [&](uint32_t c, const std::vector<Out>& outs) {
    WpCp& e = cp[c];
    for (size_t k = 0; k < outs.size(); ++k) {
      std::memcpy(e.out + e.nbytes, outs[k].bytes.data(), outs[k].bytes.size());
      e.nbytes = (uint8_t)(e.nbytes + outs[k].bytes.size());
      e.cls = (uint8_t)(e.cls | (outs[k].cls << (2 * k)));
    }
    e.nchars = (uint8_t)outs.size();
    e.covered = 1;
    nv.table[c] = outs;
  };
  for (uint32_t c = 0xE8; c <= 0xEB; ++c) set(c, {{"e", 3}});       // e with an accent -> e
  for (uint32_t c = 0xC8; c <= 0xCB; ++c) set(c, {{"e", 3}});
  set(0xDF, {{ss, 3}});
  set(0xA0, {{" ", 1}});
  set(0xAD, {});                                                      // removed
  set(0x200B, {});
  set(0x2014, {{dash, 2}});
  set(0x20AC, {{euro, 3}});
  for (uint32_t c = 0x4E00; c < 0x4E40; ++c) set(c, {{" ", 1}, {utf8(c), 3}, {" ", 1}});
  for (uint32_t c = 0xAC00; c < 0xAC00 + 28 * 4; ++c) {
    const uint32_t s = c - 0xAC00, tj = s % 28;
    std::vector<Out> o = {{utf8(0x1100 + s / 588), 3}, {utf8(0x1161 + (s % 588) / 28), 3}};
    if (tj) o.push_back({utf8(0x11A7 + tj), 3});
    set(c, o);
  }
  set(0x1100, {{g, 3}});
  set(0x1161, {{a, 3}});
  set(0x1F600, {{grin, 3}});
  const std::string e_acute = utf8(0xE9), ga = utf8(0xAC00), gag = utf8(0xAC01), nbsp = utf8(0xA0), shy = utf8(0xAD), zw = utf8(0x200B), unc = utf8(0x378);

  std::vector<std::string> rows = {"", "ab", "caf" + e_acute, "CAF" + utf8(0xC9) + " cafe", "stra" + ss + "e", "stra" + ss + "ez", euro + "5", "ab" + zhong + "ab", zhong + zhong, ga, gag,
                                   ga + ga, "ab" + nbsp + "ab", "ab" + shy + "ab", "ab" + zw + "ab", zw, "a" + dash + "b", grin, "a" + grin + "b", grin + grin,
                                   std::string(99, 'q') + ss, std::string(100, 'q') + ss, std::string(99, 'q') + ss + std::string(98, 'b') + ss, "ab" + unc, unc,
                                   utf8(0x20000), utf8(0x10FFFF), "ab\x80", "\x80", "ab\xc3", "ab\xe4\xb8", "\xc0\xaf", "\xe0\x80\xaf", "\xf0\x80\x80\xaf", "\xed\xa0\x80",
                                   "\xf8\x88\x80\x80\x80", "\xfc\x84\x80\x80\x80\x80", "\xf4\x90\x80\x80", "\xc3\xa9\xa9", "[SEP] \x80", e_acute + "[MASK]", "[MASK" + e_acute,
                                   "see [SEP] here", std::string(1 << 16, ' ') + ga, "a" + utf8(0x2192) + "b heap", utf8(0x2192), "ok" + utf8(0xE9), "k" + utf8(0xE8), "ab\xe2\x86", "\x80" + utf8(0x2192), std::string("\xa9\xa9")};
  for (const std::string& c : {ss, euro, grin, ga, zhong}) {
    std::string w;
    for (int k = 1; k <= 101; ++k) {
      w += c;
      if (k >= 99 || k == 33) rows.push_back(w);
    }
    rows.push_back(w + " " + c);
  }
  std::string many;
  for (int i = 0; i < 300; ++i) many += "ab stra" + ss + "e " + gag;
  rows.push_back(many);
  const std::vector<std::string> frag = {"ab", "heap", "cafe", " ", " ", ",", e_acute, ss, euro, zhong, ga, gag, grin, dash, nbsp, shy, zw, "Q", "z"};
  std::mt19937 rng(20260);
  for (int i = 0; i < 300; ++i) {
    std::string s;
    const size_t size = rng() % 2000;
    while (s.size() < size) s += frag[rng() % frag.size()];
    if (i % 3 == 1) s += unc;                                  // uncovered
    if (i % 3 == 2 && !s.empty()) s[rng() % s.size()] = (char)(0x80 + rng() % 0x80);  // an arbitrary byte >= 0x80: malformed more often than not
    rows.push_back(s);
  }

  int checked = 0;
  for (int lowercase = 1; lowercase >= 0; --lowercase) {
    WpHost H;
    std::string err;
    if (!wp_build(H, bytes.data(), off.data(), (int)vocab.size(), lit_bytes.data(), lit_off.data(), (int)nv.literals.size(), nv.unk, nv.cls, nv.sep, nv.max_chars, lowercase, err)) {
      std::fprintf(stderr, "wp_build: %s\n", err.c_str());
      return 1;
    }
    if (!wp_u8_check_table(cp.data(), (int)cp.size(), nv.max_chars, err)) {
      std::fprintf(stderr, "wp_u8_check_table: %s\n", err.c_str());
      return 1;
    }
    const WpU8 u{cp.data(), (int32_t)cp.size(), H.max_len0_all, H.max_len1_all, H.lit_first2, H.lit_first3};
    if (H.max_len0_all != 101 || H.t.max_len0 != 6) ++fails;  // over all entries in bytes ("q" x 99 + sharp s) / over the ASCII entries alone ("[MASK]")
    nv.lowercase = lowercase != 0;
    for (const std::string& s : rows) {
      for (int ml : {2, 3, 8, 256, 512})
        for (int special = 0; special < 2; ++special) {
          compare(H.t, u, nv, s, ml, special != 0);
          ++checked;
        }
      compare_malformed(s);
    }
    // a shorter table: the code points from n_cp on are uncovered
    const WpU8 cut{cp.data(), 0x1100, H.max_len0_all, H.max_len1_all, H.lit_first2, H.lit_first3};
    int32_t ids[8], len;
    uint8_t st;
    wp_encode_text_u8(H.t, cut, (const uint8_t*)ga.data(), (int64_t)ga.size(), 8, 1, ids, &len, &st);
    if (st != 2 || len != 0) ++fails;
    wp_encode_text_u8(H.t, cut, (const uint8_t*)ss.data(), (int64_t)ss.size(), 8, 1, ids, &len, &st);
    if (st != 0 || len != 3) ++fails;
  }
  {  // the refusals of the table check
    std::string err;
    auto refused = [&](uint32_t c, const WpCp& bad, int max_chars) {
      std::vector<WpCp> t2 = cp;
      t2[c] = bad;
      err.clear();
      if (wp_u8_check_table(t2.data(), (int)t2.size(), max_chars, err) || err.empty()) ++fails;
    };
    WpCp e = cp[0xDF];
    e.nbytes = 13; refused(0xDF, e, 100);
    e = cp[0xDF]; e.out[1] = 'x'; refused(0xDF, e, 100);                 // a lead byte without its continuation
    e = cp[0xDF]; e.cls = 0; refused(0xDF, e, 100);                      // no class
    e = cp[0xDF]; e.nchars = 2; refused(0xDF, e, 100);                   // the count is not the bytes'
    e = cp[0xDF]; e.covered = 2; refused(0xDF, e, 100);
    e = cp[0xDF]; e.out[0] = 0xED; e.out[1] = 0xA0; e.out[2] = 0x80; e.nbytes = 3; refused(0xDF, e, 100);  // a surrogate
    refused(0xDF, cp[0xDF], 190);                                        // 4 x 190 + a step's output do not fit the word buffer
    if (wp_u8_check_table(cp.data(), 0, 100, err) || wp_u8_check_table(cp.data(), WP_U8_CODE_POINTS + 1, 100, err) || wp_u8_check_table(nullptr, 16, 100, err)) ++fails;
    if (!wp_u8_check_table(cp.data(), 0x100, 100, err)) ++fails;
  }
  if (fails) {
    std::fprintf(stderr, "wordpiece_utf8_host_check: %d FAILED\n", fails);
    return 1;
  }
  std::printf("wordpiece_utf8_host_check: OK (%d rows)\n", checked);
  return 0;
}
