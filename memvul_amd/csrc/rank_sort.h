// Per-anchor ranking quality: for every vector g (an anchor of the bank, or the embedding of a fresh CVE description) the exact ROC-AUC, the average precision and
// the best-F1 cut of its P(same) over the rows of a kept corpus — rank statistics: a sort per vector, then scans.  include/memvul_rank.h states the definitions.
//
// The scores are defined bit for bit: P(same)[n, g] is the fp32 value the engine's matcher produces for that pair.  kept_terms.h states its arithmetic, sa_n and
// bv_g included, once for the four kept-corpus libraries; the score kernel here restates the ending only, instruction order as in the per-anchor claims sweep,
// and a GPU test pins the bits to the engine:
//   dd_{n,g} = fma chain of (W_c[0] - W_c[1])[i] * |u_n[i] - v_g[i]|, i ascending, from 0      (the weight differences are formed in fp32 first)
//   delta = (sa_n + bv_g) + dd;  e = expf(-|delta|);  inv = 1 / (1 + e);  P_0 = delta >= 0 ? inv : e inv;  P_1 the other;  P(same) = P_{same_idx}
//
// Plan (rank.hip drives it), per group of vectors sized to the workspace cap:
//   rank_score_kernel       the claims tile: lane = row, RK_QT vector chains per lane, the rows staged through LDS RK_MI features at a time.  The ending packs
//                           key = bits(P) << 1 | class (a NaN: RK_NAN, all ones) and stores keys [vector][row], coalesced; a row past the range stores nothing
//   rank_bank_fold_kernel   the bank slot: per row the unsigned maximum of the group's keys, folded into bank [row] BEFORE the sort permutes them
//   a segmented LSD radix sort of the group's key arrays, 8 bits x 4 passes, ascending; each pass is three launches over all vectors of the group:
//     rank_hist_kernel        per (tile, vector): the digit histogram -> hist [vector][tile][256]
//     rank_digit_scan_kernel  per vector: exclusive sum over (digit, tile), in place
//     rank_scatter_kernel     per (tile, vector): STABLE scatter; the rank inside the tile is (same-digit keys in earlier waves of the tile, from LDS counters) +
//                             (same-digit keys in lower lanes of the wave, from eight ballots)
//   statistics on the sorted keys (position i ascending; M = the keys that are not RK_NAN, which sort last):
//     rank_tile_sums_kernel   per (tile, vector): the class bits, the group starts, the live keys, the tile's last group start and the class bits below it
//     rank_tile_scan_kernel   per vector: exclusive sums over the tiles; for every tile the last group start BELOW it and the class bits below that start (a tie
//                             group may span any number of tiles: its start is propagated, never assumed to be the tile's first row); n_pos, M, D
//     rank_stats_kernel       per (tile, vector): for every position that ends a tie group, TP_g, FP_g, tp_g, fp_g from the two prefixes and the propagated start;
//                             three reductions — int64 u2 per tile, float64 ap per 256 positions in the fixed shape, the arg-max of the exact F1 compare per tile;
//                             CURVE: the group's point is written at D - (group starts at or below it)
//     rank_finish_kernel      per vector: the tiles' partials -> the result slot
// No workgroup ever waits on another: every dependency between workgroups is a launch boundary (the per-XCD L2s are not coherent, and a stuck spin hangs a shared
// machine).  No global atomics, no scratch, no assembly instruction written by hand; nothing depends on scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kept_terms.h"

#define RK_QT 16          // vectors per workgroup tile of the score kernel = chains per lane
#define RK_MI 32          // features staged per step
#define RK_BR 256         // rows per workgroup of the score kernel
#define RK_GRID_Y 1024    // row blocks per z-slice of the score kernel's grid
#define RK_NAN 0xffffffffu  // the key of a NaN score: above every other key
#define RK_CHUNK 256      // positions per ap partial: the smallest tile
#define RK_SCAN_SEGS 4    // tile segments of the digit scan's workgroup (256 digits x 4)
// the per-group workspace never exceeds this many bytes: the vectors are processed in groups sized to it (one at the least).  Per vector and row: keys ping and
// pong 8 B, histograms 1 B (tiles of 1 024), and per tile ~72 B of partials; the bank slot's key 4 B per row once.  At 1.2 M rows: 10.9 MB per vector -> groups of 96.
#define RK_WORK_CAP_BYTES (1ll << 30)

typedef float rk_f4 __attribute__((ext_vector_type(4)));

// ---- the weight differences, formed in fp32 on the device the matcher runs on: wd [3][P] = W_m[0] - W_m[1] for the W_a, W_b and W_c thirds
__global__ __launch_bounds__(256) void rank_weight_delta_kernel(const float* __restrict__ Wm, float* __restrict__ wd, int P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < 3 * P) wd[e] = Wm[e] - Wm[3 * P + e];
}

// ---- sa_n for rows [first, first + n): one wave per row, four rows per workgroup of 256
template <int P>
__global__ __launch_bounds__(256) void rank_row_term_kernel(const float* __restrict__ U, const float* __restrict__ wd, float* __restrict__ sa, long long first, long long n) {
  ks_row_term<P>(U, wd, sa, first, n);
}

// ---- one group of nq vectors v [nq][P] -> vT [P][Qs] (zeros behind nq) and bv [Qs]; one thread per slot, workgroups of 64
template <int P>
__global__ __launch_bounds__(64) void rank_vector_prep_kernel(const float* __restrict__ v, const float* __restrict__ wd, float* __restrict__ vT, float* __restrict__ bv, int nq, int Qs) {
  ks_vector_prep<P>(v, wd, vT, bv, nq, Qs);
}

struct RankScoreArgs {
  long long first, count;  // the rows in range; block b takes rows first + b RK_BR ..
  long long nblocks;       // row blocks
  int nq, Qs;              // vectors of the group and its padded width (a multiple of RK_QT)
  int same_idx;
  const uint8_t* cls;      // [N], 0 or 1
  uint32_t* keys;          // [nq][count]
};

template <int P>
__global__ __launch_bounds__(RK_BR) void rank_score_kernel(const float* __restrict__ U, const float* __restrict__ sa, const float* __restrict__ vT,
                                                           const float* __restrict__ bv, const float* __restrict__ wd, RankScoreArgs a) {
  constexpr int BR = RK_BR, STRIDE = RK_MI + 4, NST = RK_MI / 4;  // NST float4 per thread per step (BR threads stage BR rows x RK_MI features)
  static_assert(BR % 64 == 0 && P % (2 * RK_MI) == 0, "tile");
  __shared__ __attribute__((aligned(16))) float sv[BR * STRIDE];  // row chunk
  const int tid = threadIdx.x;
  // grid: x = tile of vectors (fastest), (y, z) = row block: the workgroups that read the same rows are dispatched next to each other
  const long long rb = blockIdx.y + (long long)blockIdx.z * RK_GRID_Y;
  if (rb >= a.nblocks) return;  // (the whole workgroup: the last z-slice is ragged)
  const long long r0 = rb * BR;
  const int t0 = blockIdx.x * RK_QT;  // first vector of the tile, within the group
  const float* Ub = U + (size_t)a.first * P;
  rk_f4 stage[2][NST];
  // rows past the range read its last row (never stored): a select on the address, not on the value (no branch around the loads)
#define RK_LOAD_CHUNK(ST, I0)                                                        \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (RK_MI / 4), c4 = e % (RK_MI / 4);           \
    const long long gr = r0 + r < a.count ? r0 + r : a.count - 1;                    \
    stage[ST][j] = *(const rk_f4*)(Ub + (size_t)gr * P + (I0) + 4 * c4);             \
  }
#define RK_STORE_CHUNK(ST)                                                           \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (RK_MI / 4), c4 = e % (RK_MI / 4);           \
    *(rk_f4*)(sv + r * STRIDE + 4 * c4) = stage[ST][j];                              \
  }
  float dd[RK_QT];
#pragma unroll
  for (int j = 0; j < RK_QT; ++j) dd[j] = 0.f;
  const float* myrow = sv + tid * STRIDE;
  const float* wc = wd + 2 * P;
  const float* vt = vT + t0;
  // Left alone, hipcc pairs neighbouring chains into packed fp32 instructions, which have no |x| source modifier (a v_and per value) and are no faster per value
  // than the plain forms.  An EMPTY asm statement that names the sixteen values keeps them scalar; it emits no instruction of its own.
  static_assert(RK_QT == 16, "RK_OPAQUE16 names sixteen values");
#define RK_OPAQUE16(X)                                                                                                                   \
  asm("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]), "+v"(X[6]), "+v"(X[7]), "+v"(X[8]), "+v"(X[9]), \
           "+v"(X[10]), "+v"(X[11]), "+v"(X[12]), "+v"(X[13]), "+v"(X[14]), "+v"(X[15]));
  // one chunk: every lane walks its row's RK_MI features in ascending order; per feature the RK_QT vector values and the weight are wave-uniform
#define RK_COMPUTE(I0)                                                               \
  _Pragma("unroll 1") for (int q = 0; q < RK_MI / 4; ++q) {                          \
    const rk_f4 uu = *(const rk_f4*)(myrow + 4 * q);                                 \
    const float* vq = vt + (size_t)((I0) + 4 * q) * a.Qs;                            \
    const float* wq = wc + (I0) + 4 * q;                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
      const float wv = wq[e];                                                        \
      float t[RK_QT];                                                                \
      _Pragma("unroll") for (int j = 0; j < RK_QT; ++j) t[j] = uu[e] - vq[(size_t)e * a.Qs + j]; \
      RK_OPAQUE16(t)                                                                 \
      _Pragma("unroll") for (int j = 0; j < RK_QT; ++j) dd[j] = fmaf(wv, fabsf(t[j]), dd[j]);    \
      RK_OPAQUE16(dd)                                                                \
    }                                                                                \
  }
  RK_LOAD_CHUNK(0, 0)
  RK_LOAD_CHUNK(1, RK_MI)
#pragma unroll 1
  for (int i0 = 0; i0 < P; i0 += 2 * RK_MI) {  // two chunks per trip: `stage` keeps compile-time indices and stays in registers
    RK_STORE_CHUNK(0)
    __syncthreads();
    if (i0 + 2 * RK_MI < P) { RK_LOAD_CHUNK(0, i0 + 2 * RK_MI) }
    RK_COMPUTE(i0)
    __syncthreads();  // every wave is done with this chunk before the next one overwrites it
    RK_STORE_CHUNK(1)
    __syncthreads();
    if (i0 + 3 * RK_MI < P) { RK_LOAD_CHUNK(1, i0 + 3 * RK_MI) }
    RK_COMPUTE(i0 + RK_MI)
    __syncthreads();
  }
#undef RK_LOAD_CHUNK
#undef RK_STORE_CHUNK
#undef RK_COMPUTE
#undef RK_OPAQUE16
  // ---- softmax_2 of the class difference, as the engine's matcher forms it; then the key
  const long long rr = r0 + tid;
  const bool live = rr < a.count;
  const float sar = sa[a.first + (live ? rr : a.count - 1)];
  const uint32_t c = a.cls[a.first + (live ? rr : a.count - 1)] != 0 ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < RK_QT; ++j) {
    const float dl = (sar + bv[t0 + j]) + dd[j];
    const float ed = expf(-fabsf(dl));
    const float inv = 1.0f / (1.0f + ed);
    const float p0 = dl >= 0.f ? inv : ed * inv, p1 = dl >= 0.f ? ed * inv : inv;
    const float p = a.same_idx == 0 ? p0 : p1;
    const uint32_t key = p != p ? RK_NAN : ((__float_as_uint(p) << 1) | c);
    if (live && t0 + j < a.nq) a.keys[(size_t)(t0 + j) * a.count + rr] = key;
  }
}

// ---- bank [row] = max(bank [row], the group's keys of the row); first: the group is the call's first, bank holds nothing yet
__global__ __launch_bounds__(256) void rank_bank_fold_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ bank, long long count, int nq, int first) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= count) return;
  uint32_t m = first ? 0u : bank[r];
  for (int q = 0; q < nq; ++q) {
    const uint32_t k = keys[(size_t)q * count + r];
    m = k > m ? k : m;
  }
  bank[r] = m;
}

// ---- one pass of the sort.  keys [nq][count]; hist [nq][ntiles][256]; grid (ntiles, nq), TR threads: thread = position of the tile

template <int TR>
__global__ __launch_bounds__(TR) void rank_hist_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ hist, int count, int shift) {
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.y;
  const int pos = blockIdx.x * TR + tid;
  if (tid < 256) h[tid] = 0;
  __syncthreads();
  if (pos < count) atomicAdd(&h[(keys[q * count + pos] >> shift) & 255u], 1u);  // (LDS, inside the workgroup: a count, whatever the order)
  __syncthreads();
  if (tid < 256) hist[(q * gridDim.x + blockIdx.x) * 256 + tid] = h[tid];
}

// hist [nq][ntiles][256] counts -> the first output position of every (digit, tile), digits outermost: one workgroup per vector, thread = (segment of the
// tiles, digit); the loads of a step are 256 consecutive counts
__global__ __launch_bounds__(256 * RK_SCAN_SEGS) void rank_digit_scan_kernel(uint32_t* __restrict__ hist, int ntiles) {
  __shared__ uint32_t seg_sum[RK_SCAN_SEGS][256];
  __shared__ uint32_t base[256];
  const int d = threadIdx.x & 255, s = threadIdx.x >> 8;
  uint32_t* hq = hist + (size_t)blockIdx.x * ntiles * 256;
  const int per = (ntiles + RK_SCAN_SEGS - 1) / RK_SCAN_SEGS;
  const int t0 = s * per < ntiles ? s * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  uint32_t sum = 0;
  for (int t = t0; t < t1; ++t) sum += hq[(size_t)t * 256 + d];
  seg_sum[s][d] = sum;
  __syncthreads();
  if (s == 0) {  // the digit's total
    uint32_t tot = 0;
#pragma unroll
    for (int i = 0; i < RK_SCAN_SEGS; ++i) tot += seg_sum[i][d];
    base[d] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t below = 0;
    for (int i = 0; i < 256; ++i) {
      const uint32_t x = base[i];
      base[i] = below;
      below += x;
    }
  }
  __syncthreads();
  uint32_t run = base[d];
  for (int i = 0; i < s; ++i) run += seg_sum[i][d];
  for (int t = t0; t < t1; ++t) {
    const uint32_t x = hq[(size_t)t * 256 + d];
    hq[(size_t)t * 256 + d] = run;
    run += x;
  }
}

template <int TR>
__global__ __launch_bounds__(TR) void rank_scatter_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ hist, int count,
                                                          int shift) {
  constexpr int NW = TR / 64;
  __shared__ uint32_t wcnt[NW][256];  // per wave and digit: the wave's keys of that digit, then the first output position of them
  const int tid = threadIdx.x, w = tid >> 6;
  const size_t q = blockIdx.y;
  const int pos = blockIdx.x * TR + tid;
  for (int i = tid; i < NW * 256; i += TR) (&wcnt[0][0])[i] = 0;
  const bool live = pos < count;
  const uint32_t key = live ? in[q * count + pos] : 0u;
  const uint32_t d = (key >> shift) & 255u;
  // the lanes of the wave that hold the same digit: eight ballots
  unsigned long long same = __ballot(live);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned long long set = __ballot(live && ((d >> b) & 1u));
    same &= ((d >> b) & 1u) ? set : ~set;
  }
  const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));  // same-digit lanes below this one
  __syncthreads();
  if (live && below == 0) wcnt[w][d] = (uint32_t)__popcll(same);
  __syncthreads();
  if (tid < 256) {
    uint32_t run = hist[(q * gridDim.x + blockIdx.x) * 256 + tid];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const uint32_t x = wcnt[i][tid];
      wcnt[i][tid] = run;
      run += x;
    }
  }
  __syncthreads();
  if (live) {
    const uint32_t dest = wcnt[w][d] + below;
    if (dest < (uint32_t)count) out[q * count + dest] = key;  // (always, when the histogram is this pass's)
  }
}

// ---- statistics on the sorted keys

struct RankTileSum {  // per (vector, tile)
  int cls, starts, live;  // class bits, group starts, keys that are not RK_NAN
  int last;               // the tile's last group start, as position in the tile + 1; 0: none
  int below;              // class bits of the tile below that start
};
struct RankTileCarry {  // per (vector, tile): what lies below the tile
  int cls, starts;        // class bits and group starts
  int start, start_cls;   // the last group start (a position of the vector) and the class bits below it
};
struct RankTotals {  // per vector
  int n_pos, live, groups;
};
struct RankBest {  // a cut: (TP, FP) at the threshold of key >> 1
  uint32_t tp, fp, key;
};

// a is the better cut: the higher F1 = 2 TP / (TP + FP + n_pos), compared exactly; equal F1: the higher threshold
__device__ __forceinline__ bool rk_better(const RankBest a, const RankBest b, uint32_t n_pos) {
  const unsigned __int128 l = (unsigned __int128)a.tp * ((unsigned long long)b.tp + b.fp + n_pos);
  const unsigned __int128 r = (unsigned __int128)b.tp * ((unsigned long long)a.tp + a.fp + n_pos);
  return l > r || (l == r && a.key > b.key);
}

// inclusive scans over the TR threads of a workgroup (sum / max of ints); part: LDS [TR / 64]
template <int TR, bool MAX>
__device__ __forceinline__ int rk_block_scan(int x, int* part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const int y = __shfl_up(x, dlt, 64);
    if (lane >= dlt) x = MAX ? (y > x ? y : x) : x + y;
  }
  __syncthreads();  // (part is free again)
  if (lane == 63) part[w] = x;
  __syncthreads();
  int below = 0;
#pragma unroll
  for (int i = 0; i < TR / 64; ++i)
    if (i < w) below = MAX ? (part[i] > below ? part[i] : below) : below + part[i];
  return MAX ? (below > x ? below : x) : x + below;
}

// what a thread knows of its position: the key, whether it is live, starts a tie group, ends one
struct RankPos {
  uint32_t key;
  bool live, start, end;
};
__device__ __forceinline__ RankPos rk_position(const uint32_t* __restrict__ kq, int pos, int count) {
  RankPos p;
  p.key = pos < count ? kq[pos] : RK_NAN;
  p.live = p.key != RK_NAN;
  const uint32_t prev = pos > 0 && pos < count ? kq[pos - 1] : RK_NAN, next = pos + 1 < count ? kq[pos + 1] : RK_NAN;
  p.start = p.live && (pos == 0 || (prev >> 1) != (p.key >> 1));
  p.end = p.live && (next >> 1) != (p.key >> 1);  // (RK_NAN >> 1 is no score's bit pattern)
  return p;
}

template <int TR>
__global__ __launch_bounds__(TR) void rank_tile_sums_kernel(const uint32_t* __restrict__ keys, RankTileSum* __restrict__ sums, int count) {
  __shared__ int part[TR / 64];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.y;
  const RankPos p = rk_position(keys + q * count, blockIdx.x * TR + tid, count);
  const int c = p.live ? (int)(p.key & 1u) : 0;
  const int cls = rk_block_scan<TR, false>(c, part);
  const int starts = rk_block_scan<TR, false>(p.start ? 1 : 0, part);
  const int live = rk_block_scan<TR, false>(p.live ? 1 : 0, part);
  const int last = rk_block_scan<TR, true>(p.start ? tid + 1 : 0, part);
  // (the last thread holds the tile's totals; every thread must know `last` of the whole tile for the next sum)
  __shared__ int tile_last;
  if (tid == TR - 1) tile_last = last;
  __syncthreads();
  const int below = rk_block_scan<TR, false>(tid + 1 < tile_last ? c : 0, part);
  if (tid == TR - 1) {
    RankTileSum s;
    s.cls = cls; s.starts = starts; s.live = live; s.last = last; s.below = below;
    sums[q * gridDim.x + blockIdx.x] = s;
  }
}

// one workgroup per vector; every thread a run of consecutive tiles
template <int TR>
__global__ __launch_bounds__(256) void rank_tile_scan_kernel(const RankTileSum* __restrict__ sums, RankTileCarry* __restrict__ carry, RankTotals* __restrict__ totals,
                                                             int ntiles) {
  __shared__ int r_cls[256], r_starts[256], r_live[256], r_start[256], r_scls[256];
  const int tid = threadIdx.x;
  const RankTileSum* sq = sums + (size_t)blockIdx.x * ntiles;
  RankTileCarry* cq = carry + (size_t)blockIdx.x * ntiles;
  const int per = (ntiles + 255) / 256;
  const int t0 = tid * per < ntiles ? tid * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  int cls = 0, starts = 0, live = 0;
  for (int t = t0; t < t1; ++t) {
    cls += sq[t].cls;
    starts += sq[t].starts;
    live += sq[t].live;
  }
  r_cls[tid] = cls; r_starts[tid] = starts; r_live[tid] = live;
  __syncthreads();
  if (tid == 0) {
    int a = 0, b = 0, c = 0;
    for (int i = 0; i < 256; ++i) {
      const int x = r_cls[i], y = r_starts[i], z = r_live[i];
      r_cls[i] = a; r_starts[i] = b;
      a += x; b += y; c += z;
    }
    RankTotals tt;
    tt.n_pos = a; tt.groups = b; tt.live = c;
    totals[blockIdx.x] = tt;
  }
  __syncthreads();
  // the run's last group start (position + 1; 0: none) and the class bits below it
  cls = r_cls[tid];
  int start = 0, scls = 0;
  for (int t = t0; t < t1; ++t) {
    const RankTileSum s = sq[t];
    if (s.last) {
      start = t * TR + s.last;
      scls = cls + s.below;
    }
    cls += s.cls;
  }
  r_start[tid] = start; r_scls[tid] = scls;
  __syncthreads();
  if (tid == 0) {
    int a = 0, b = 0;
    for (int i = 0; i < 256; ++i) {
      const int x = r_start[i], y = r_scls[i];
      r_start[i] = a; r_scls[i] = b;
      if (x) { a = x; b = y; }
    }
  }
  __syncthreads();
  cls = r_cls[tid]; starts = r_starts[tid]; start = r_start[tid]; scls = r_scls[tid];
  for (int t = t0; t < t1; ++t) {
    const RankTileSum s = sq[t];
    RankTileCarry c;
    c.cls = cls; c.starts = starts; c.start = start - 1; c.start_cls = scls;  // (start - 1 = -1 only for tile 0, whose first live position is a start)
    cq[t] = c;
    if (s.last) {
      start = t * TR + s.last;
      scls = cls + s.below;
    }
    cls += s.cls;
    starts += s.starts;
  }
}

struct RankStatsArgs {
  const uint32_t* keys;        // [nq][count], sorted
  const RankTileCarry* carry;  // [nq][ntiles]
  const RankTotals* totals;    // [nq]
  long long* u2;               // [nq][ntiles]
  double* ap;                  // [nq][nchunks]
  RankBest* best;              // [nq][ntiles]
  float* c_thres;              // CURVE: [groups]
  long long *c_tp, *c_fp;
  int count, nchunks;
};

template <int TR, bool CURVE>
__global__ __launch_bounds__(TR) void rank_stats_kernel(RankStatsArgs a) {
  constexpr int NW = TR / 64;
  __shared__ int part[NW];
  __shared__ int ex[TR];  // class bits below each position of the tile (of the whole vector)
  __shared__ long long w_u2[NW];
  __shared__ double w_ap[NW];
  __shared__ RankBest w_best[NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t q = blockIdx.y;
  const int ntiles = gridDim.x;
  const int pos = blockIdx.x * TR + tid;
  const RankPos p = rk_position(a.keys + q * a.count, pos, a.count);
  const RankTileCarry cy = a.carry[q * ntiles + blockIdx.x];
  const RankTotals tt = a.totals[q];
  const int c = p.live ? (int)(p.key & 1u) : 0;
  const int cpos = cy.cls + rk_block_scan<TR, false>(c, part);  // class bits at or below the position
  ex[tid] = cpos - c;
  const int gi = cy.starts + rk_block_scan<TR, false>(p.start ? 1 : 0, part);  // group starts at or below it
  const int ls = rk_block_scan<TR, true>(p.start ? tid + 1 : 0, part);         // the last one's place in the tile + 1 (the scans' barriers cover ex)
  const int s = ls ? blockIdx.x * TR + ls - 1 : cy.start;
  const int below = ls ? ex[ls - 1] : cy.start_cls;  // the positives below the group
  const int n_pos = tt.n_pos, n_neg = tt.live - tt.n_pos;
  long long u2 = 0;
  double ap = 0.0;
  RankBest best = {0u, 0u, 0u};
  if (p.end) {
    const long long tp_g = cpos - below, fp_g = (long long)(pos - s + 1) - tp_g;
    const long long TP = n_pos - below, FP = (long long)(tt.live - s) - TP;
    u2 = tp_g * (2 * ((long long)n_neg - FP) + fp_g);
    ap = ((double)tp_g / (double)n_pos) * ((double)TP / (double)(TP + FP));
    best.tp = (uint32_t)TP; best.fp = (uint32_t)FP; best.key = p.key;
    if constexpr (CURVE) {
      const int at = tt.groups - gi;  // thresholds descending
      if (at >= 0 && at < tt.groups) {  // (always)
        a.c_thres[at] = __uint_as_float(p.key >> 1);
        a.c_tp[at] = TP;
        a.c_fp[at] = FP;
      }
    }
  }
  // the wave's 64 positions by a butterfly (both partners of a step form the same sum), then the waves in order
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    u2 += __shfl_xor(u2, m, 64);
    ap += __shfl_xor(ap, m, 64);
    RankBest o;
    o.tp = __shfl_xor(best.tp, m, 64); o.fp = __shfl_xor(best.fp, m, 64); o.key = __shfl_xor(best.key, m, 64);
    if (rk_better(o, best, (uint32_t)n_pos)) best = o;
  }
  if (lane == 0) { w_u2[w] = u2; w_ap[w] = ap; w_best[w] = best; }
  __syncthreads();
  if (tid < TR / RK_CHUNK) {  // four waves per 256 positions, left to right
    const int chunk = blockIdx.x * (TR / RK_CHUNK) + tid;
    if (chunk < a.nchunks) a.ap[q * a.nchunks + chunk] = ((w_ap[4 * tid] + w_ap[4 * tid + 1]) + w_ap[4 * tid + 2]) + w_ap[4 * tid + 3];
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < NW; ++i) {
      u2 += w_u2[i];
      if (rk_better(w_best[i], best, (uint32_t)n_pos)) best = w_best[i];
    }
    a.u2[q * ntiles + blockIdx.x] = u2;
    a.best[q * ntiles + blockIdx.x] = best;
  }
}

// the result slots, [slots] each
struct RankOut {
  long long* n;       // [slots][3]: n_neg, n_pos, n_nan
  long long* u2;
  double* ap;
  float* best_thres;
  long long* best;    // [slots][2]: TP, FP
};

// one workgroup per vector: the tiles' partials -> slot slot0 + vector.  ap: accumulator t takes the 256-blocks t, t + 256, .. in ascending order, then a halving tree
__global__ __launch_bounds__(256) void rank_finish_kernel(const RankTotals* __restrict__ totals, const long long* __restrict__ u2, const double* __restrict__ ap,
                                                          const RankBest* __restrict__ best, int ntiles, int nchunks, int count, int slot0, RankOut out) {
  __shared__ long long s_u2[256];
  __shared__ double s_ap[256];
  __shared__ RankBest s_best[256];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const RankTotals tt = totals[q];
  long long u = 0;
  double x = 0.0;
  RankBest b = {0u, 0u, 0u};
  for (int t = tid; t < ntiles; t += 256) {
    u += u2[q * ntiles + t];
    const RankBest o = best[q * ntiles + t];
    if (rk_better(o, b, (uint32_t)tt.n_pos)) b = o;
  }
  for (int c = tid; c < nchunks; c += 256) x += ap[q * nchunks + c];
  s_u2[tid] = u; s_ap[tid] = x; s_best[tid] = b;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (tid < half) {
      s_u2[tid] += s_u2[tid + half];
      s_ap[tid] += s_ap[tid + half];
      if (rk_better(s_best[tid + half], s_best[tid], (uint32_t)tt.n_pos)) s_best[tid] = s_best[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const size_t o = (size_t)slot0 + q;
    const bool none = tt.n_pos == 0;
    out.n[3 * o] = tt.live - tt.n_pos;
    out.n[3 * o + 1] = tt.n_pos;
    out.n[3 * o + 2] = count - tt.live;
    out.u2[o] = none ? 0 : s_u2[0];
    out.ap[o] = none ? __builtin_nan("") : s_ap[0];
    out.best_thres[o] = none ? __builtin_nanf("") : __uint_as_float(s_best[0].key >> 1);
    out.best[2 * o] = none ? 0 : (long long)s_best[0].tp;
    out.best[2 * o + 1] = none ? 0 : (long long)s_best[0].fp;
  }
}
