// Per-anchor claims: for every vector g (an anchor of the bank, or the embedding of a fresh CVE description) EVERY row of a kept corpus whose P(same) reaches a
// threshold — the reference's decision rule (prob >= thres), not a rank — and, per vector and threshold, how many rows of each class it claims.
//
// The result is defined bit for bit: P(same)[n, g] is the fp32 value the engine's matcher (match_topk.h) produces for that pair.  kept_terms.h states its arithmetic,
// sa_n and bv_g included, once for the four kept-corpus libraries;
// a pair is CLAIMED iff P(same) >= t in IEEE fp32: a NaN claims nothing (the per-anchor top-k library ranks a NaN first; here it is never listed and never counted).
//
// Plan (claims.hip drives it):
//   claim_row_term_kernel     sa_n, once per row when the row is added: one wave per row
//   claim_vector_prep_kernel  per group of vectors: bv_g, and the vectors transposed to vT [P][Qs] (Qs = the group padded to CL_QT, zeros behind it), so that the CL_QT
//                             values of one feature are consecutive dwords: a wave-uniform operand the compiler fetches by one scalar load
//   claim_score_kernel        lane = row; a workgroup = BR rows x CL_QT vectors.  The rows are staged through LDS CL_MI features at a time by coalesced 16-byte
//                             loads, two chunks ahead (row stride CL_MI + 4 floats: the lane = row ds_read_b128 is conflict-free); every staged u value meets the
//                             CL_QT chains a lane keeps in registers: 2 VALU operations (v_sub, v_fma with |x| as a source modifier) per (row, vector, feature).
//                             Rows are numbered from the range's first row, so a wave's 64 rows are one 64-bit word of the range whatever `first` is.  The ending:
//     CL_COUNT  per threshold t and vector, one ballot (P >= t) per wave; its population count, and that of its AND with the wave's class ballot, land in lane t
//               of a register, the waves' registers are summed in LDS, and the block stores one packed word (class 0 | class 1 << 16) per
//               (vector, threshold): partials [vector][block][T]
//     CL_MARK   one ballot per vector (its own threshold) -> the bit matrix [vector][ceil(count / 64)]
//     CL_FILL   tiles whose words are all zero return at once; the others are scored again (the same instructions, so the same bits) and every claimed lane writes
//               its row and P(same) at offsets[vector] + base[vector][word] + (set bits below the lane): ascending rows, no atomics, no dependence on scheduling
//   claim_fold_kernel         a SEPARATE launch sums a vector's partials over the blocks into int64 [Q][T][2].  (Nothing is combined across workgroups inside the
//                             score kernel: the per-XCD L2s are not coherent, and match_topk.h records what the fences cost.  Integer sums are exact in any order.)
//   claim_scan_kernel         per vector: the words' population counts -> the base of every word (exclusive sum) and the vector's total
// No atomics, no scratch, no assembly instruction written by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kept_terms.h"

#define CL_QT 16          // vectors per workgroup tile = chains per lane
#define CL_MI 32          // features staged per step
#define CL_TMAX 64        // thresholds per counts call: one lane of a wave each
#define CL_GRID_Y 1024    // row blocks per z-slice of the score kernel's grid (z <= 32 768 at 2^31 rows in blocks of 64)
#define CL_FOLD_WAVES 16  // waves of the fold kernel's workgroup: wave w sums blocks w, w + 16, ..
// the per-group workspace never exceeds this many bytes: the vectors are processed in groups sized to it (one tile of CL_QT at the least).  counts: partials
// [group][blocks][T] x 4 B — at 1.2 M rows, 256 rows per block, T = 40: 4 688 blocks x 160 B = 750 KB per vector -> groups of 352.  select: the bit matrix and the
// word bases, 12 B per 64 rows — 225 KB per vector at 1.2 M rows -> G = 1000 is one group.
#define CL_WORK_CAP_BYTES (256ll << 20)

#define CL_COUNT 0
#define CL_MARK 1
#define CL_FILL 2

typedef float cl_f4 __attribute__((ext_vector_type(4)));

// ---- the weight differences, formed in fp32 on the device the matcher runs on: wd [3][P] = W_m[0] - W_m[1] for the W_a, W_b and W_c thirds
__global__ __launch_bounds__(256) void claim_weight_delta_kernel(const float* __restrict__ Wm, float* __restrict__ wd, int P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < 3 * P) wd[e] = Wm[e] - Wm[3 * P + e];
}

// ---- sa_n for rows [first, first + n): one wave per row
template <int P>
__global__ __launch_bounds__(256) void claim_row_term_kernel(const float* __restrict__ U, const float* __restrict__ wd, float* __restrict__ sa, long long first, long long n) {
  ks_row_term<P>(U, wd, sa, first, n);
}

// ---- one group of nq vectors v [nq][P] -> vT [P][Qs] (zeros behind nq) and bv [Qs]; one thread per slot
template <int P>
__global__ __launch_bounds__(64) void claim_vector_prep_kernel(const float* __restrict__ v, const float* __restrict__ wd, float* __restrict__ vT, float* __restrict__ bv, int nq, int Qs) {
  ks_vector_prep<P>(v, wd, vT, bv, nq, Qs);
}

struct ClaimScoreArgs {
  long long first, count;      // the rows in range; block b takes rows first + b BR ..
  long long nblocks, W;        // row blocks; words per vector = ceil(count / 64)
  int nq, Qs, q0;              // vectors of the group, its padded width (a multiple of CL_QT), and the group's first vector
  int same_idx, T;
  const float* thr;            // CL_COUNT: [T]; CL_MARK: [Q], one per vector
  const uint8_t* cls;          // [N], 0 or 1
  uint32_t* part;              // CL_COUNT: [nq][nblocks][T], class 0 | class 1 << 16
  unsigned long long* bits;    // CL_MARK writes, CL_FILL reads: [nq][W]
  const uint32_t* wbase;       // CL_FILL: [nq][W], claimed rows of the vector below the word
  const long long* offs;       // CL_FILL: [Q + 1]
  long long total;             // CL_FILL: offs[Q]
  long long* rows;             // CL_FILL: [total]
  float* p;
};

template <int P, int BR, int MODE>
__global__ __launch_bounds__(BR) void claim_score_kernel(const float* __restrict__ U, const float* __restrict__ sa, const float* __restrict__ vT,
                                                         const float* __restrict__ bv, const float* __restrict__ wd, ClaimScoreArgs a) {
  constexpr int NW = BR / 64, STRIDE = CL_MI + 4, NST = CL_MI / 4;  // NST float4 per thread per step (BR threads stage BR rows x CL_MI features)
  static_assert(BR % 64 == 0 && P % (2 * CL_MI) == 0 && NW * CL_QT * 64 <= BR * STRIDE && CL_QT * NW <= 128, "tile");
  __shared__ __attribute__((aligned(16))) float sv[BR * STRIDE];  // row chunk; later CL_COUNT's per-wave counts [NW][CL_QT][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // grid: x = tile of vectors (fastest), (y, z) = row block: the workgroups that read the same rows are dispatched next to each other
  const long long rb = blockIdx.y + (long long)blockIdx.z * CL_GRID_Y;
  if (rb >= a.nblocks) return;  // (the whole workgroup: the last z-slice is ragged)
  const long long r0 = rb * BR;
  const int t0 = blockIdx.x * CL_QT;  // first vector of the tile, within the group
  const long long widx = rb * NW + w; // this wave's word of the range
  if constexpr (MODE == CL_FILL) {    // a tile that claims nothing has nothing to write: every wave looks at all of the tile's words and decides alike
    bool any = false;
#pragma unroll
    for (int i = lane; i < CL_QT * NW; i += 64) {
      const int j = i / NW;
      const long long wi = rb * NW + i % NW;
      if (t0 + j < a.nq && wi < a.W) any = any || a.bits[(size_t)(t0 + j) * a.W + wi] != 0ull;
    }
    if (__ballot(any) == 0ull) return;
  }
  const float* Ub = U + (size_t)a.first * P;
  cl_f4 stage[2][NST];
  // rows past the range read its last row (never claimed, never counted): a select on the address, not on the value (no branch around the loads)
#define CL_LOAD_CHUNK(ST, I0)                                                        \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (CL_MI / 4), c4 = e % (CL_MI / 4);           \
    const long long gr = r0 + r < a.count ? r0 + r : a.count - 1;                    \
    stage[ST][j] = *(const cl_f4*)(Ub + (size_t)gr * P + (I0) + 4 * c4);             \
  }
#define CL_STORE_CHUNK(ST)                                                           \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (CL_MI / 4), c4 = e % (CL_MI / 4);           \
    *(cl_f4*)(sv + r * STRIDE + 4 * c4) = stage[ST][j];                              \
  }
  float dd[CL_QT];
#pragma unroll
  for (int j = 0; j < CL_QT; ++j) dd[j] = 0.f;
  const float* myrow = sv + tid * STRIDE;
  const float* wc = wd + 2 * P;
  const float* vt = vT + t0;
  // Left alone, hipcc pairs neighbouring chains into v_pk_add_f32 / v_pk_fma_f32, which have no |x| source modifier (a v_and per value) and are no faster per
  // value than the plain forms (match_topk.h, tools/valu_rate.hip).  An EMPTY asm statement that names the sixteen values keeps them scalar; it emits no
  // instruction of its own.
  static_assert(CL_QT == 16, "CL_OPAQUE16 names sixteen values");
#define CL_OPAQUE16(X)                                                                                                                   \
  asm("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]), "+v"(X[6]), "+v"(X[7]), "+v"(X[8]), "+v"(X[9]), \
           "+v"(X[10]), "+v"(X[11]), "+v"(X[12]), "+v"(X[13]), "+v"(X[14]), "+v"(X[15]));
  // one chunk: every lane walks its row's CL_MI features in ascending order; per feature the CL_QT vector values and the weight are wave-uniform
#define CL_COMPUTE(I0)                                                               \
  _Pragma("unroll 1") for (int q = 0; q < CL_MI / 4; ++q) {                          \
    const cl_f4 uu = *(const cl_f4*)(myrow + 4 * q);                                 \
    const float* vq = vt + (size_t)((I0) + 4 * q) * a.Qs;                            \
    const float* wq = wc + (I0) + 4 * q;                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
      const float wv = wq[e];                                                        \
      float t[CL_QT];                                                                \
      _Pragma("unroll") for (int j = 0; j < CL_QT; ++j) t[j] = uu[e] - vq[(size_t)e * a.Qs + j]; \
      CL_OPAQUE16(t)                                                                 \
      _Pragma("unroll") for (int j = 0; j < CL_QT; ++j) dd[j] = fmaf(wv, fabsf(t[j]), dd[j]);    \
      CL_OPAQUE16(dd)                                                                \
    }                                                                                \
  }
  CL_LOAD_CHUNK(0, 0)
  CL_LOAD_CHUNK(1, CL_MI)
#pragma unroll 1
  for (int i0 = 0; i0 < P; i0 += 2 * CL_MI) {  // two chunks per trip: `stage` keeps compile-time indices and stays in registers
    CL_STORE_CHUNK(0)
    __syncthreads();
    if (i0 + 2 * CL_MI < P) { CL_LOAD_CHUNK(0, i0 + 2 * CL_MI) }
    CL_COMPUTE(i0)
    __syncthreads();  // every wave is done with this chunk before the next one overwrites it
    CL_STORE_CHUNK(1)
    __syncthreads();
    if (i0 + 3 * CL_MI < P) { CL_LOAD_CHUNK(1, i0 + 3 * CL_MI) }
    CL_COMPUTE(i0 + CL_MI)
    __syncthreads();
  }
#undef CL_LOAD_CHUNK
#undef CL_STORE_CHUNK
#undef CL_COMPUTE
#undef CL_OPAQUE16
  // ---- softmax_2 of the class difference, as match_topk.h forms it; a lane past the range holds a NaN, which claims nothing
  const long long rr = r0 + tid;
  const bool live = rr < a.count;
  const float sar = sa[a.first + (live ? rr : a.count - 1)];
  float ps[CL_QT];
#pragma unroll
  for (int j = 0; j < CL_QT; ++j) {
    const float dl = (sar + bv[t0 + j]) + dd[j];
    const float ed = expf(-fabsf(dl));
    const float inv = 1.0f / (1.0f + ed);
    const float p0 = dl >= 0.f ? inv : ed * inv, p1 = dl >= 0.f ? ed * inv : inv;
    ps[j] = live ? (a.same_idx == 0 ? p0 : p1) : __builtin_nanf("");
  }
  if constexpr (MODE == CL_COUNT) {
    const unsigned long long cw = __ballot(live && a.cls[a.first + (live ? rr : 0)] != 0);  // the wave's rows of class 1
    int acc[CL_QT];  // lane t: the wave's rows claimed at threshold t, class 0 | class 1 << 16
#pragma unroll
    for (int j = 0; j < CL_QT; ++j) acc[j] = 0;
    for (int t = 0; t < a.T; ++t) {
      const float th = a.thr[t];
#pragma unroll
      for (int j = 0; j < CL_QT; ++j) {
        const unsigned long long word = __ballot(ps[j] >= th);
        const int n1 = __popcll(word & cw), n = __popcll(word);
        const int both = __builtin_amdgcn_readfirstlane((n - n1) | (n1 << 16));  // (wave-uniform: formed once, ahead of the lane select)
        acc[j] = lane == t ? both : acc[j];
      }
    }
    // (the staging loop ended on a barrier: sv is free)  per-wave counts -> LDS, then one thread per (vector, threshold) sums the waves: at most 512 per half
    int* cnt = (int*)sv;
#pragma unroll
    for (int j = 0; j < CL_QT; ++j) cnt[(w * CL_QT + j) * 64 + lane] = acc[j];
    __syncthreads();
    for (int i = tid; i < CL_QT * 64; i += BR) {
      const int j = i >> 6, t = i & 63;
      int s = 0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) s += cnt[(ww * CL_QT + j) * 64 + t];
      if (t < a.T && t0 + j < a.nq) a.part[((size_t)(t0 + j) * a.nblocks + rb) * a.T + t] = (uint32_t)s;
    }
  } else if constexpr (MODE == CL_MARK) {
    int lo = 0, hi = 0;  // lane j: the wave's word of vector t0 + j
#pragma unroll
    for (int j = 0; j < CL_QT; ++j) {
      const int q = a.q0 + t0 + (t0 + j < a.nq ? j : 0);  // (a padded slot reads a threshold that exists; its word is not stored)
      const unsigned long long word = __ballot(ps[j] >= a.thr[q]);
      lo = lane == j ? (int)(unsigned)word : lo;
      hi = lane == j ? (int)(unsigned)(word >> 32) : hi;
    }
    if (lane < CL_QT && t0 + lane < a.nq && widx < a.W) a.bits[(size_t)(t0 + lane) * a.W + widx] = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  } else {
    if (widx >= a.W) return;  // (a wave wholly past the range)
#pragma unroll
    for (int j = 0; j < CL_QT; ++j) {
      if (t0 + j >= a.nq) break;
      const size_t wo = (size_t)(t0 + j) * a.W + widx;
      const unsigned long long word = a.bits[wo];
      if (live && ((word >> lane) & 1ull)) {
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
        const long long o = a.offs[a.q0 + t0 + j] + a.wbase[wo] + below;
        if (o < a.total) {
          a.rows[o] = a.first + rr;
          a.p[o] = ps[j];
        }
      }
    }
  }
}

// ---- partials [nq][nblocks][T] -> counts [Q][T][2] (this group's vectors from q0 on), int64: one workgroup per vector, lane = threshold, wave w takes blocks
// w, w + CL_FOLD_WAVES, ..; the waves' sums meet in LDS
__global__ __launch_bounds__(64 * CL_FOLD_WAVES) void claim_fold_kernel(const uint32_t* __restrict__ part, long long* __restrict__ counts, long long nblocks, int T, int q0) {
  __shared__ long long s0[CL_FOLD_WAVES][64], s1[CL_FOLD_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t q = blockIdx.x;
  long long c0 = 0, c1 = 0;
  if (lane < T)
    for (long long b = w; b < nblocks; b += CL_FOLD_WAVES) {
      const uint32_t x = part[(q * nblocks + b) * T + lane];
      c0 += x & 0xffffu;
      c1 += x >> 16;
    }
  s0[w][lane] = c0;
  s1[w][lane] = c1;
  __syncthreads();
  if (w == 0 && lane < T) {
    c0 = c1 = 0;
#pragma unroll
    for (int ww = 0; ww < CL_FOLD_WAVES; ++ww) {
      c0 += s0[ww][lane];
      c1 += s1[ww][lane];
    }
    counts[((size_t)q0 + q) * T * 2 + 2 * lane] = c0;
    counts[((size_t)q0 + q) * T * 2 + 2 * lane + 1] = c1;
  }
}

// ---- bits [nq][W] -> wbase [nq][W] (claimed rows of the vector below each word) and totals [Q] (this group's vectors from q0 on): one workgroup per vector,
// every thread a run of consecutive words
__global__ __launch_bounds__(256) void claim_scan_kernel(const unsigned long long* __restrict__ bits, uint32_t* __restrict__ wbase, long long* __restrict__ totals,
                                                         long long W, int q0) {
  __shared__ uint32_t run[256];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const long long per = (W + 255) / 256;
  const long long w0 = tid * per < W ? tid * per : W, w1 = w0 + per < W ? w0 + per : W;
  uint32_t s = 0;  // (a vector claims fewer than 2^31 rows)
  for (long long i = w0; i < w1; ++i) s += (uint32_t)__popcll(bits[q * W + i]);
  run[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t below = 0;
    for (int i = 0; i < 256; ++i) {
      const uint32_t x = run[i];
      run[i] = below;
      below += x;
    }
    totals[q0 + q] = (long long)below;
  }
  __syncthreads();
  uint32_t base = run[tid];
  for (long long i = w0; i < w1; ++i) {
    wbase[q * W + i] = base;
    base += (uint32_t)__popcll(bits[q * W + i]);
  }
}
