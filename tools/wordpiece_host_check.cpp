// The host core of memvul_amd/csrc/wordpiece.h under the sanitizers: a stand-alone program (its own main; nothing here is loaded into python or needs a GPU).
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I memvul_amd/csrc tools/wordpiece_host_check.cpp -o wordpiece_host_check
//   ./wordpiece_host_check            -> "wordpiece_host_check: OK (<rows> rows)" and exit status 0
// It builds the table for a small vocabulary, runs the edge table and 200 fuzz rows through wp_encode_text at several max_length values, with and without the
// special tokens, and compares every row with a naive restatement of the rule over std::map and std::string (longest candidate first, as WordPiece is usually
// written) — so the sanitizers see every path of the table builder, the probe, the matcher and the driver, and a disagreement fails the run too.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "wordpiece.h"

namespace {

struct Naive {
  std::map<std::string, int> vocab;
  std::vector<std::string> literals;
  int unk, cls, sep, max_chars;
  bool lowercase;

  void word(const std::string& w, std::vector<int>& out) const {
    if ((int)w.size() > max_chars) { out.push_back(unk); return; }
    std::vector<int> pieces;
    size_t start = 0;
    while (start < w.size()) {
      size_t end = w.size();
      int id = -1;
      for (; end > start; --end) {
        auto it = vocab.find((start ? "##" : "") + w.substr(start, end - start));
        if (it != vocab.end()) { id = it->second; break; }
      }
      if (id < 0) { out.push_back(unk); return; }
      pieces.push_back(id);
      start = end;
    }
    out.insert(out.end(), pieces.begin(), pieces.end());
  }

  // ids (without padding) or status 1
  bool encode(const std::string& s, int max_length, bool special, std::vector<int>& ids) const {
    ids.clear();
    for (unsigned char c : s)
      if (c >= 0x80) return false;
    for (const std::string& l : literals)
      if (s.find(l) != std::string::npos) return false;
    std::vector<int> toks;
    std::string w;
    for (unsigned char c : s) {
      const bool ws = c == 9 || c == 10 || c == 13 || c == 32;
      if (!ws && (c < 32 || c == 127)) continue;
      const bool punct = (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126);
      if (ws || punct) {
        if (!w.empty()) word(w, toks);
        w.clear();
        if (punct) word(std::string(1, (char)c), toks);
      } else {
        w.push_back((char)((lowercase && c >= 'A' && c <= 'Z') ? c + 32 : c));
      }
    }
    if (!w.empty()) word(w, toks);
    const size_t budget = (size_t)(max_length - (special ? 2 : 0));
    if (toks.size() > budget) toks.resize(budget);
    if (special) ids.push_back(cls);
    ids.insert(ids.end(), toks.begin(), toks.end());
    if (special) ids.push_back(sep);
    return true;
  }
};

int fails = 0;

void compare(const WpTable& t, const Naive& nv, const std::string& s, int max_length, bool special) {
  std::vector<int32_t> ids((size_t)max_length, 12345);
  int32_t len = -7;
  uint8_t status = 9;
  wp_encode_text(t, (const uint8_t*)s.data(), (int64_t)s.size(), max_length, special ? 1 : 0, ids.data(), &len, &status);
  std::vector<int> want;
  const bool ours = nv.encode(s, max_length, special, want);
  bool ok = status == (ours ? 0 : 1) && len == (int32_t)want.size();
  for (int i = 0; ok && i < max_length; ++i) ok = ids[(size_t)i] == (i < (int)want.size() ? want[(size_t)i] : 0);
  if (!ok && fails++ < 5) std::fprintf(stderr, "MISMATCH max_length %d special %d len %d want %zu status %d text[%zu] %.60s\n", max_length, (int)special, len, want.size(), status, s.size(), s.c_str());
}

}  // namespace

int main() {
  std::vector<std::string> vocab = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"};
  for (char c = 'a'; c < 'z'; ++c) { vocab.push_back(std::string(1, c)); vocab.push_back(std::string("##") + c); }
  for (char c = '0'; c <= '9'; ++c) vocab.push_back(std::string(1, c));
  for (int c = 33; c < 126; ++c)
    if ((c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || c >= 123) vocab.push_back(std::string(1, (char)c));
  for (const char* w : {"ab", "abab", "buffer", "overflow", "over", "heap", "the", "un", "##able", "##ing", "##flow", "##ab", "##abab", "stack", "caf\xc3\xa9", "##"})
    vocab.push_back(w);
  vocab.push_back(std::string(100, 'q'));
  vocab.push_back("##" + std::string(99, 'b'));
  vocab.push_back(std::string(150, 'k'));  // longer than max_chars: left out of the table, never matched
  vocab.push_back("");                      // an unused id
  std::string bytes, lit_bytes;
  std::vector<int64_t> off{0}, lit_off{0};
  Naive nv;
  for (size_t k = 0; k < vocab.size(); ++k) {
    bytes += vocab[k];
    off.push_back((int64_t)bytes.size());
    if (!vocab[k].empty()) nv.vocab[vocab[k]] = (int)k;
  }
  nv.literals = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"};
  for (const std::string& l : nv.literals) { lit_bytes += l; lit_off.push_back((int64_t)lit_bytes.size()); }
  nv.unk = 1; nv.cls = 2; nv.sep = 3; nv.max_chars = 100;

  std::vector<std::string> rows;
  for (int c = 0; c < 128; ++c) rows.push_back(std::string("ab") + (char)c + "ab");
  rows.insert(rows.end(), {std::string(99, 'q'), std::string(100, 'q'), std::string(101, 'q'), std::string(100, 'a') + std::string(99, 'b'),
                           std::string(100, 'a') + std::string(100, 'b'), std::string(100, 'q') + std::string(99, 'b'), "abz", "bufferz overflow", "", " ", " \t\n\r ",
                           "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~", "Buffer OVERFLOW in HeAp", std::string(1 << 20, ' ') + "heap", std::string(100000, 'a'),
                           "see [SEP] here", "see[MASK]here", "[sep]", "[CLS", "[CLS]", "ab\x80", std::string(150, 'k'), "unable overflowing heaps", "[MAS", "x[", "["});
  std::string many;
  for (int i = 0; i < 600; ++i) many += "ab heapabab ";
  rows.push_back(many);
  std::mt19937 rng(20250);
  for (int i = 0; i < 200; ++i) {
    std::string s((size_t)(rng() % 3001), ' ');
    for (char& c : s) c = (char)(rng() % 128);
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
    nv.lowercase = lowercase != 0;
    for (const std::string& s : rows)
      for (int ml : {2, 3, 8, 12, 256, 512})
        for (int special = 0; special < 2; ++special) {
          if (s.size() > 50000 && ml != 8 && ml != 512) continue;
          compare(H.t, nv, s, ml, special != 0);
          ++checked;
        }
  }
  {  // the refusals of the builder
    WpHost H;
    std::string err;
    if (wp_build(H, bytes.data(), off.data(), (int)vocab.size(), lit_bytes.data(), lit_off.data(), 5, 1, 2, 3, 191, 1, err) || err.empty()) ++fails;
    if (wp_build(H, bytes.data(), off.data(), 0, lit_bytes.data(), lit_off.data(), 5, 1, 2, 3, 100, 1, err)) ++fails;
    if (wp_build(H, bytes.data(), off.data(), (int)vocab.size(), lit_bytes.data(), lit_off.data(), 5, (int)vocab.size(), 2, 3, 100, 1, err)) ++fails;
  }
  if (fails) {
    std::fprintf(stderr, "wordpiece_host_check: %d FAILED\n", fails);
    return 1;
  }
  std::printf("wordpiece_host_check: OK (%d rows)\n", checked);
  return 0;
}
