// Per-anchor retrieval: for every query vector g (an anchor of the bank, or the embedding of a fresh CVE description) the k best-matching rows of a kept
// corpus — the TRANSPOSE of match_topk.h, which ranks anchors per row.  Here N (rows) >> Q (query vectors).
//
// The result is defined bit for bit: P(same)[n, g] is the fp32 value the engine's matcher (match_topk.h) produces for that pair.  kept_terms.h states its arithmetic,
// sa_n and bv_g included, once for the four kept-corpus libraries.
// ranking per g: (rt_key(P) descending, row ascending), rt_key(NaN) = 2.0.
//
// Plan (retrieve.hip drives it):
//   report_row_term_kernel   sa_n, once per row when the row is added: one wave per row
//   report_query_prep_kernel per group of query vectors: bv_g, and the vectors transposed to vT [P][Qs] (Qs = the group padded to RT_QT, zeros behind it), so that the
//                            RT_QT values of one feature are consecutive dwords: a wave-uniform operand the compiler fetches by one scalar load
//   report_score_kernel      lane = row; a workgroup = BR rows x RT_QT query vectors.  The rows are staged through LDS RT_MI features at a time by coalesced 16-byte
//                            loads, two chunks ahead (row stride RT_MI + 4 floats: the lane = row ds_read_b128 is conflict-free); every staged u value meets the
//                            RT_QT chains a lane keeps in registers: 2 VALU operations (v_sub, v_fma with |x| as a source modifier) per (row, vector, feature), the
//                            vector and weight operands from SGPRs.  The block's P(same) tile goes to LDS and one wave per query vector selects the block's k best
//                            in k rounds of a 64-bit wave maximum -> candidate lists [Q][blocks][k]  (or, for mvr_psame, the tile goes straight to memory)
//   report_merge_kernel      SEPARATE launches fold fan_in lists into one until one is left; the last writes the result.  (Nothing is merged across workgroups
//                            inside the score kernel: the per-XCD L2s are not coherent, and match_topk.h records what the fences cost.)
// No atomics, no scratch, no assembly instruction written by hand.  Cost, as a MODEL from instruction counts (nothing measured): N Q P 2 / 64 wave-instructions = 2.4 G at N = 1.2 M,
// Q = 124, P = 512 — a few milliseconds chip-wide at the ~2 ns per wave-instruction per SIMD tools/valu_rate.hip measured for plain fp32 forms; the rows are
// read from HBM about once per group of query vectors (the tiles of one row block run next to each other).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kept_terms.h"

#define RT_KMAX 64
#define RT_QT 16          // query vectors per workgroup tile = chains per lane
#define RT_MI 32          // features staged per step
#define RT_NOROW 0x7fffffff
#define RT_GRID_Y 1024    // row blocks per z-slice of the score kernel's grid (z <= 32 768 at 2^31 rows in blocks of 64)
// the candidate lists [group][blocks][k] x (fp32 P, int32 row) never exceed this many bytes: the query vectors are processed in groups sized to it (one tile of
// RT_QT at the least).  At the 1.2 M-row shard of BASELINE configs[3], k = 64, 256 rows per block: 4 688 blocks x 512 B = 2.4 MB per vector -> groups of 96; G = 1000 fits.
#define RT_LIST_CAP_BYTES (256ll << 20)

typedef float rt_f4 __attribute__((ext_vector_type(4)));

// rank key: NaN ranks above every probability (match_topk.h mk_key)
__device__ __forceinline__ float rt_key(float x) { return x != x ? 2.0f : x; }

// Wave-wide maximum of one 64-bit word per lane, every lane gets it (the same ladder)
__device__ __forceinline__ unsigned long long rt_wave_max64(unsigned long long x) {
#define RT_MAX_STEP(CTRL, ROWS)                                                                     \
  {                                                                                                 \
    const unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);                                      \
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, ROWS, 0xf, false); \
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, ROWS, 0xf, false); \
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;                             \
    x = o > x ? o : x;                                                                              \
  }
  RT_MAX_STEP(0x111, 0xf)
  RT_MAX_STEP(0x112, 0xf)
  RT_MAX_STEP(0x114, 0xf)
  RT_MAX_STEP(0x118, 0xf)
  RT_MAX_STEP(0x142, 0xa)
  RT_MAX_STEP(0x143, 0xc)
#undef RT_MAX_STEP
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// A candidate is ONE word (key bits << 32) | ~row: keys are >= 0 as floats, so their bit patterns order like the values, and ~row lets the lower row win a tie.
// An exhausted slot (row RT_NOROW) is 0 and ranks below everything.
__device__ __forceinline__ unsigned long long rt_word(float p, int row) {
  return row == RT_NOROW ? 0ull : ((unsigned long long)__float_as_uint(fmaxf(rt_key(p), 0.0f)) << 32) | (unsigned)(~row);
}

// k rounds of arg-max over candidates held NJ per lane (candidate j of lane l = slot l + 64 j).  emit(round, slot): the winner's slot, or -1 when the candidates
// are exhausted; every lane calls it with the same arguments.  Rows differ, so a round's winner is unique.
template <int NJ, typename F>
__device__ __forceinline__ void rt_select(const unsigned long long (&cand)[NJ], int k, int lane, F emit) {
  unsigned long long prev = ~0ull;
  for (int round = 0; round < k; ++round) {
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const unsigned long long c = cand[j];
      best = (c < prev && c > best) ? c : best;
    }
    best = rt_wave_max64(best);
    int slot = -1;
#pragma unroll
    for (int j = 0; j < NJ; ++j) slot = (best != 0ull && cand[j] == best) ? lane + 64 * j : slot;
    const unsigned long long has = __ballot(slot >= 0);
    const int src = has ? __ffsll((long long)has) - 1 : 0;
    slot = __builtin_amdgcn_readlane(slot, src);
    emit(round, best == 0ull ? -1 : slot);
    prev = best;  // (0 once exhausted: nothing is below it)
  }
}

// ---- the weight differences, formed in fp32 on the device the matcher runs on: wd [3][P] = W_m[0] - W_m[1] for the W_a, W_b and W_c thirds
__global__ __launch_bounds__(256) void report_weight_delta_kernel(const float* __restrict__ Wm, float* __restrict__ wd, int P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < 3 * P) wd[e] = Wm[e] - Wm[3 * P + e];
}

// ---- sa_n for rows [first, first + n): one wave per row
template <int P>
__global__ __launch_bounds__(256) void report_row_term_kernel(const float* __restrict__ U, const float* __restrict__ wd, float* __restrict__ sa, long long first, long long n) {
  ks_row_term<P>(U, wd, sa, first, n);
}

// ---- one group of nq query vectors v [nq][P] -> vT [P][Qs] (zeros behind nq) and bv [Qs]; one thread per slot
template <int P>
__global__ __launch_bounds__(64) void report_query_prep_kernel(const float* __restrict__ v, const float* __restrict__ wd, float* __restrict__ vT, float* __restrict__ bv, int nq, int Qs) {
  ks_vector_prep<P>(v, wd, vT, bv, nq, Qs);
}

struct ReportScoreArgs {
  long long first, count;  // the rows in range; block b takes rows first + b BR ..
  int nq, Qs;              // query vectors of the group, and its padded width (a multiple of RT_QT)
  int same_idx, k;
  long long nblocks;       // row blocks = lists per query vector
  float* part_p;           // [nq][nblocks][k]
  int32_t* part_row;
  float* psame;            // PSAME build: [count][Q], this group's columns from q0 on
  int Q, q0;
};

template <int P, int BR, int PSAME>
__global__ __launch_bounds__(BR) void report_score_kernel(const float* __restrict__ U, const float* __restrict__ sa, const float* __restrict__ vT,
                                                          const float* __restrict__ bv, const float* __restrict__ wd, ReportScoreArgs a) {
  constexpr int NW = BR / 64, STRIDE = RT_MI + 4, NST = RT_MI / 4;  // NST float4 per thread per step (BR threads stage BR rows x RT_MI features)
  static_assert(BR % 64 == 0 && P % (2 * RT_MI) == 0 && RT_QT * BR <= BR * STRIDE, "tile");
  __shared__ __attribute__((aligned(16))) float sv[BR * STRIDE];  // row chunk; later the P(same) tile [RT_QT][BR]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // grid: x = tile of query vectors (fastest), (y, z) = row block: the workgroups that read the same rows are dispatched next to each other, so the rows come from
  // HBM about once per group of vectors and from the caches for the other tiles (2.5 GB of rows do not stay there from one tile's sweep to the next)
  const long long rb = blockIdx.y + (long long)blockIdx.z * RT_GRID_Y;
  if (rb >= a.nblocks) return;  // (the whole workgroup: the last z-slice is ragged)
  const long long r0 = rb * BR;
  const int t0 = blockIdx.x * RT_QT;  // first query vector of the tile
  const float* Ub = U + (size_t)a.first * P;
  rt_f4 stage[2][NST];
  // rows past the range read its last row (never ranked, never stored): a select on the address, not on the value (no branch around the loads)
#define RT_LOAD_CHUNK(ST, I0)                                                        \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (RT_MI / 4), c4 = e % (RT_MI / 4);           \
    const long long gr = r0 + r < a.count ? r0 + r : a.count - 1;                    \
    stage[ST][j] = *(const rt_f4*)(Ub + (size_t)gr * P + (I0) + 4 * c4);             \
  }
#define RT_STORE_CHUNK(ST)                                                           \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (RT_MI / 4), c4 = e % (RT_MI / 4);           \
    *(rt_f4*)(sv + r * STRIDE + 4 * c4) = stage[ST][j];                              \
  }
  float dd[RT_QT];
#pragma unroll
  for (int j = 0; j < RT_QT; ++j) dd[j] = 0.f;
  const float* myrow = sv + tid * STRIDE;
  const float* wc = wd + 2 * P;
  const float* vt = vT + t0;
  // Left alone, hipcc pairs neighbouring chains into v_pk_add_f32 / v_pk_fma_f32, which have no |x| source modifier (a v_and per value) and are no faster per
  // value than the plain forms (match_topk.h, tools/valu_rate.hip).  An EMPTY asm statement that names the sixteen values keeps them scalar; it emits no
  // instruction of its own (hipcc follows it with one s_nop: two per 32 VALU operations).
  static_assert(RT_QT == 16, "RT_OPAQUE16 names sixteen values");
#define RT_OPAQUE16(X)                                                                                                                   \
  asm("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]), "+v"(X[6]), "+v"(X[7]), "+v"(X[8]), "+v"(X[9]), \
           "+v"(X[10]), "+v"(X[11]), "+v"(X[12]), "+v"(X[13]), "+v"(X[14]), "+v"(X[15]));
  // one chunk: every lane walks its row's RT_MI features in ascending order; per feature the RT_QT vector values and the weight are wave-uniform
#define RT_COMPUTE(I0)                                                               \
  _Pragma("unroll 1") for (int q = 0; q < RT_MI / 4; ++q) {                          \
    const rt_f4 uu = *(const rt_f4*)(myrow + 4 * q);                                 \
    const float* vq = vt + (size_t)((I0) + 4 * q) * a.Qs;                            \
    const float* wq = wc + (I0) + 4 * q;                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
      const float wv = wq[e];                                                        \
      float t[RT_QT];                                                                \
      _Pragma("unroll") for (int j = 0; j < RT_QT; ++j) t[j] = uu[e] - vq[(size_t)e * a.Qs + j]; \
      RT_OPAQUE16(t)                                                                 \
      _Pragma("unroll") for (int j = 0; j < RT_QT; ++j) dd[j] = fmaf(wv, fabsf(t[j]), dd[j]);    \
      RT_OPAQUE16(dd)                                                                \
    }                                                                                \
  }
  RT_LOAD_CHUNK(0, 0)
  RT_LOAD_CHUNK(1, RT_MI)
#pragma unroll 1
  for (int i0 = 0; i0 < P; i0 += 2 * RT_MI) {  // two chunks per trip: `stage` keeps compile-time indices and stays in registers
    RT_STORE_CHUNK(0)
    __syncthreads();
    if (i0 + 2 * RT_MI < P) { RT_LOAD_CHUNK(0, i0 + 2 * RT_MI) }
    RT_COMPUTE(i0)
    __syncthreads();  // every wave is done with this chunk before the next one overwrites it
    RT_STORE_CHUNK(1)
    __syncthreads();
    if (i0 + 3 * RT_MI < P) { RT_LOAD_CHUNK(1, i0 + 3 * RT_MI) }
    RT_COMPUTE(i0 + RT_MI)
    __syncthreads();
  }
#undef RT_LOAD_CHUNK
#undef RT_STORE_CHUNK
#undef RT_COMPUTE
#undef RT_OPAQUE16
  // ---- softmax_2 of the class difference, as match_topk.h forms it
  const long long rr = r0 + tid;
  const bool live = rr < a.count;
  const float sar = sa[a.first + (live ? rr : a.count - 1)];
  float* sp = sv;  // [RT_QT][BR]
#pragma unroll
  for (int j = 0; j < RT_QT; ++j) {
    const float dl = (sar + bv[t0 + j]) + dd[j];
    const float ed = expf(-fabsf(dl));
    const float inv = 1.0f / (1.0f + ed);
    const float p0 = dl >= 0.f ? inv : ed * inv, p1 = dl >= 0.f ? ed * inv : inv;
    const float ps = a.same_idx == 0 ? p0 : p1;
    if constexpr (PSAME) {
      if (live && t0 + j < a.nq) a.psame[(size_t)rr * a.Q + a.q0 + t0 + j] = ps;
    } else {
      sp[j * BR + tid] = ps;
    }
  }
  if constexpr (PSAME) return;
  __syncthreads();
  // ---- selection: wave w ranks the tile's vectors w, w + NW, ..
  for (int j = w; j < RT_QT; j += NW) {
    const int q = t0 + j;
    if (q >= a.nq) break;
    unsigned long long cand[NW];
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      const long long g = r0 + lane + 64 * c;
      cand[c] = rt_word(sp[j * BR + lane + 64 * c], g < a.count ? (int)(a.first + g) : RT_NOROW);
    }
    int won = -1;  // lane `round` remembers the round's winner; the k entries are then written by k lanes at once
    rt_select<NW>(cand, a.k, lane, [&](int round, int slot) { won = lane == round ? slot : won; });
    if (lane < a.k) {
      const size_t o = ((size_t)q * a.nblocks + rb) * a.k + lane;
      a.part_p[o] = won >= 0 ? sp[j * BR + won] : -1.0f;
      a.part_row[o] = won >= 0 ? (int)(a.first + r0 + won) : RT_NOROW;
    }
  }
}

// ---- fold fan_in lists into one: lists [nq][L_in][k] -> [nq][L_out][k], L_out = ceil(L_in / fan_in); one wave per (query vector, output list).  Each input list
// holds the k best of its rows in order, so their union holds the k best of all of them.  last (L_out == 1): the result goes to top_p / top_row instead, exhausted
// slots as p = -1, row = -1.
struct ReportMergeArgs {
  int nq, k, fan_in, last;
  long long L_in, L_out;
  const float* in_p;
  const int32_t* in_row;
  float* out_p;
  int32_t* out_row;
  float* top_p;        // [Q][k], this group's rows from q0 on
  long long* top_row;
  int q0;
};

template <int NJ>
__global__ __launch_bounds__(256) void report_merge_kernel(ReportMergeArgs a) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long long)a.nq * a.L_out) return;
  const long long q = item / a.L_out, lo = item % a.L_out;
  const long long l0 = lo * a.fan_in;
  const int nl = (int)(a.L_in - l0 < a.fan_in ? a.L_in - l0 : a.fan_in);
  const int n = nl * a.k;  // <= 64 NJ (host-enforced)
  const size_t base = ((size_t)q * a.L_in + l0) * a.k;
  float pv[NJ];
  int rv[NJ];
  unsigned long long cand[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    const int cc = c < n ? c : 0;
    pv[j] = a.in_p[base + cc];
    rv[j] = c < n ? a.in_row[base + cc] : RT_NOROW;
    cand[j] = rt_word(pv[j], rv[j]);
  }
  rt_select<NJ>(cand, a.k, lane, [&](int round, int slot) {
    if (lane != (slot >= 0 ? (slot & 63) : 0)) return;  // the winner's lane writes the round's entry
    float p = -1.0f;
    int row = RT_NOROW;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (slot >= 0 && (slot >> 6) == j) { p = pv[j]; row = rv[j]; }
    if (a.last) {
      const size_t o = (size_t)(a.q0 + q) * a.k + round;
      a.top_p[o] = p;
      a.top_row[o] = row == RT_NOROW ? -1ll : (long long)row;
    } else {
      const size_t o = ((size_t)q * a.L_out + lo) * a.k + round;
      a.out_p[o] = p;
      a.out_row[o] = row;
    }
  });
}
