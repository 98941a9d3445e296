// The sink census (include/memvul_hip.h mv_sink_census_enable / mv_sink_census_read): WHICH token the heads the concentration monitor flags sit on.
// A reader of planes the pass already holds — launched after a layer's QKV projection, next to the attention launch that feeds the monitor, it changes no
// other kernel: Q row 0 and the K rows of [B][12][S][64] fp16 (1/8 folded into Q; the hi planes, in every form), `lens`, and the pass's token ids.
//
// One wave per (sequence, head), load shape as attention_cls_kernel (attention.h): lane = (row lane >> 3, 16-B chunk lane & 7), one load instruction covers
// eight whole 128-B K rows, the 8 lanes of a row combine with three xor-shuffles.  The score of row 8 it + (lane >> 3) stays in the registers of lane chunk
// it & 7 (slot it >> 3: at most 8 per lane at S = 512), so K is read once.  All arithmetic fp32; rows >= len are left out.
//
// "Ordinary" is what the monitor means (attention_v2.h AttnArgs::conc): in ENGINE ROW ORDER rows 0 and 1 hold [CLS] and the last token, and row len - 1
// holds token 1 (misc_kernels.h embed_ln_kernel swaps them for sequences of >= 3 tokens), so the ordinary keys are rows 2 .. len - 1 = token positions
// 1 .. len - 2.  The id buffer of a pass, as checked in embed_ln_kernel: it is in NATURAL token order ([row b][position], `pitch` ints between rows — the
// kernel permutes while it reads, ids[b * pitch + ss]), so the winning ROW is mapped back to its token position (row len - 1 -> position 1) before the id is
// looked up.  Ties go to the lowest token position.  Sequences of fewer than 16 tokens are skipped (the monitor's gate).
//
// For an item whose collision mass exceeds MV_SINK_COLLISION one lane adds, with vector atomics on integers only (the result does not depend on scheduling,
// batching or streams): items[id] += 1, share_q20[id] += round(p* 2^20), by_head[layer][head] += 1.
#pragma once
#include "attention.h"

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(256) void sink_census_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k, const int32_t* __restrict__ lens,
                                                          const int32_t* __restrict__ ids, int pitch, int S_in, int S, int nbh, int vocab,
                                                          uint32_t* __restrict__ items, unsigned long long* __restrict__ share_q20,
                                                          uint32_t* __restrict__ by_head_layer) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = blockIdx.x * 4 + wave;
  if (bh >= nbh) return;  // no workgroup barrier below: waves are independent
  const int b = bh / MV_HEADS, h = bh - b * MV_HEADS;
  const int len = lens[b];
  if (len < 16) return;
  const int c = lane & 7, sub = lane >> 3;
  const half_t* qb = q + (size_t)bh * S * MV_HEAD_DIM + 8 * c;  // row 0: the [CLS] query
  const half8_t qh = *(const half8_t*)qb;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = (float)qh[e];
  const half_t* kb = k + (size_t)bh * S * MV_HEAD_DIM + (size_t)sub * MV_HEAD_DIM + 8 * c;
  const int nj = S >> 6;  // slots in use: 64 rows each
  float sc[8];            // slot j: the score of row 64 j + 8 c + sub
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = -3.0e38f;
    if (j < nj) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const half8_t kk = *(const half8_t*)(kb + (size_t)(64 * j + 8 * t) * MV_HEAD_DIM);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = __builtin_fmaf(qv[e], (float)kk[e], s);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        sc[j] = (t == c) ? s : sc[j];
      }
    }
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = 64 * j + 8 * c + sub;
    if (row >= len) sc[j] = -3.0e38f;
    mx = fmaxf(mx, sc[j]);
  }
  mx = wave_max(mx);
  float psum = 0.f, c2 = 0.f, best = -1.f;
  int best_pos = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = 64 * j + 8 * c + sub;
    const bool valid = row < len;
    const float e = valid ? __expf(sc[j] - mx) : 0.f;
    psum += e;
    if (valid && row >= 2) {  // an ordinary key
      c2 = __builtin_fmaf(e, e, c2);
      const int pos = (row == len - 1) ? 1 : row;  // the token position this row holds
      if (e > best || (e == best && pos < best_pos)) { best = e; best_pos = pos; }
    }
  }
  psum = wave_sum(psum);
  c2 = wave_sum(c2);
  const float top = wave_max(best);
  const int pos = wave_min_i32(best == top ? best_pos : 0x7fffffff);
  const float inv = 1.0f / psum;
  const float coll = c2 * inv * inv;
  if (lane == 0 && coll > MV_SINK_COLLISION && pos < len && pos < S_in) {
    const int id = ids[(size_t)b * pitch + pos];
    if (id >= 0 && id < vocab) {
      atomicAdd(items + id, 1u);
      atomicAdd(share_q20 + id, (unsigned long long)__float2uint_rn(top * inv * 1048576.0f));
      atomicAdd(by_head_layer + h, 1u);
    }
  }
}
