// Sink-token routing (include/memvul_hip.h mv_set_sink_tokens): a sequence is ROUTED iff one of its tokens at positions 1 .. len - 2 is in the handle's
// sink-token list.  Positions 0 and len - 1 are [CLS] / [SEP] (the special rows cover them; the census looks at the same positions: sink_census.h), ids at
// positions >= len are padding and are never looked at (a list with id 0 does not route by padding), and there is no length gate: len <= 2 has no such position.
// A length outside [0, S] is read as clamped to it.
//
// Two restatements of the one rule, over a vocabulary bitmap of ceil(vocab / 32) dwords (bit id & 31 of dword id >> 5):
//   route_scan          the host's, on a [B][S] id matrix — what the batch entry points and mv_route_scan run;
//   route_flags_kernel  the device's, on the resident corpus, whose ids live only there and whose list may change after the upload.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

inline std::vector<uint32_t> route_bitmap(const int32_t* tokens, int n, int vocab) {
  std::vector<uint32_t> bm(((size_t)vocab + 31) / 32, 0u);
  for (int i = 0; i < n; ++i) bm[(size_t)tokens[i] >> 5] |= 1u << (tokens[i] & 31);
  return bm;
}

// flags[b] = 1 / 0 for rows [0, B) of ids [B][S]; returns how many are routed
inline int route_scan(const int32_t* ids, const int32_t* lens, int B, int S, const uint32_t* bitmap, int vocab, uint8_t* flags) {
  int routed = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* row = ids + (size_t)b * S;
    const int len = lens[b] < 0 ? 0 : (lens[b] > S ? S : lens[b]);
    uint32_t hit = 0;
    for (int p = 1; p < len - 1; ++p) {
      const uint32_t id = (uint32_t)row[p];
      if (id < (uint32_t)vocab) hit |= (bitmap[id >> 5] >> (id & 31)) & 1u;
    }
    flags[b] = (uint8_t)hit;
    routed += (int)hit;
  }
  return routed;
}

#ifdef __HIPCC__
// One wave per corpus row (4 rows per workgroup, no barrier: the waves are independent).  The lanes stride over the 16-byte chunks that cover positions
// 1 .. len - 2 of the row; the chunks are aligned in the ARRAY (element index % 4 == 0, the allocation is), not in the row, so any pitch S works: a chunk's
// elements outside the row's window are masked, and the one chunk that would reach past the array's last element (n S % 4 != 0) is read element by element.
// Each id is tested against the bitmap in global memory (3.8 KB at BERT's vocabulary: cache-resident), a wave-wide any-reduce decides the row, lane 0 writes
// its byte.  Plain vector loads and stores; no LDS, no atomics, no scratch.
__global__ __launch_bounds__(256) void route_flags_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, int64_t n, int S,
                                                          const uint32_t* __restrict__ bitmap, int vocab, uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  int len = lens[row];
  len = len < 0 ? 0 : (len > S ? S : len);
  const int64_t lo = row * S + 1, hi = row * S + len - 1, total = n * S;  // the window [lo, hi) in elements of the array
  bool hit = false;
  if (hi > lo) {
    const int64_t c0 = lo >> 2, c1 = (hi - 1) >> 2;
    for (int64_t c = c0 + lane; c <= c1; c += 64) {
      const int64_t e = c << 2;
      int v[4];
      if (e + 4 <= total) {
        const int4 q = *(const int4*)(ids + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = e + i < total ? ids[e + i] : -1;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t id = (uint32_t)v[i];
        if (e + i >= lo && e + i < hi && id < (uint32_t)vocab) hit |= (bitmap[id >> 5] >> (id & 31)) & 1u;
      }
    }
  }
  const bool any = __ballot(hit) != 0;
  if (lane == 0) flags[row] = any ? 1 : 0;
}
#endif
