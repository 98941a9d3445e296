// Anchor-bank audit: what a bank of vectors (anchors, candidate anchors) decides AS A WHOLE over a kept corpus once each vector has its own threshold.  Everything is
// a population count over ANDs of rows and columns of one bit matrix, the marking B [Q][W] (W = ceil(count / 64) words per vector, rows numbered from the range's
// first row): B[q][n] = P(same)[n, q] >= thres[q] in IEEE fp32 (a NaN claims nothing).  Only integers leave the device.
//
// P(same)[n, g] is, bit for bit, the fp32 value the engine's matcher produces for the pair: kept_terms.h states its arithmetic, sa_n and bv_g included, once for the
// four kept-corpus libraries (this library includes no header of another library of this tree, whose kernels it would otherwise instantiate).
//
// Plan (bank.hip drives it):
//   bank_row_term_kernel      sa_n, once per row when the row is added: one wave per row
//   bank_vector_prep_kernel   per group of vectors: bv_g, and the vectors transposed to vT [P][Qs] (Qs = the group padded to BK_QT, zeros behind it)
//   bank_mark_kernel          lane = row; a workgroup = BR rows x BK_QT vectors; the rows are staged through LDS BK_MI features at a time, two chunks ahead; every
//                             staged u value meets the BK_QT chains a lane keeps in registers.  The ending: one ballot per (wave, vector) at the vector's own
//                             threshold -> its word of the group's slice of B.  Lanes past the range hold a NaN and claim nothing.
//   bank_class_words_kernel   the class bytes of the range -> posword [W] (bit l of word w = row first + 64 w + l is of class 1), once per marking
//   bank_totals_kernel        per vector: popcount(B & posword), popcount(B & ~posword) over its words -> claimed [Q][2]; one workgroup per vector
//   bank_multiplicity_kernel  a workgroup owns `chunk` consecutive words (every fetched line of B is used whole), a wave takes one word at a time with lane = row and
//                             walks the Q rows of B: m += bit, the last claimant remembered.  The class-split histogram and the sole counts are summed in LDS and
//                             the non-zero entries are added to the int64 results by integer atomics; mult / sole_of are plain coalesced stores
//   bank_overlap_kernel       a bit-matrix product: a tile of BK_OT x BK_OT vectors (upper triangle of tiles only; in a diagonal tile only q <= r) x chunks of BK_OW
//                             words staged in LDS, popcount(a & b & posword) and popcount(a & b) per pair in registers over the workgroup's words, then one integer
//                             atomic pair per (q, r); bank_mirror_kernel, a SEPARATE launch, copies the upper triangle below the diagonal
//   bank_gain_kernel          per round, grid (vector, word chunk): popcounts of B[q] & ~covered split by posword -> partials [Q][chunks][2] (plain stores)
//   bank_pick_kernel          ONE workgroup: sums each candidate's partials, gain = w_pos newpos - w_neg newneg in int64, reduces by (gain descending, index ascending),
//                             records the pick and ORs its row into `covered`; a pick with gain <= 0, the round limit or an empty field sets a sticky `done` word
//                             that turns every later launch of the two into a no-op, so the result does not depend on how often the host looks
// Nothing is read from another workgroup's stores inside one launch: sums across workgroups go through integer atomics (exact in any order) or a later launch.
// No scratch, no assembly instruction written by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kept_terms.h"

#define BK_QT 16          // vectors per workgroup tile of the mark kernel = chains per lane
#define BK_MI 32          // features staged per step
#define BK_GRID_Y 1024    // row blocks per z-slice of the mark kernel's grid
#define BK_QMAX 4096      // vectors per marking (MVB_MAX_VECTORS)
#define BK_OT 32          // overlap: vectors per tile side
#define BK_OW 64          // overlap: words staged per step
#define BK_PICK_THREADS 1024

typedef float bk_f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long bk_u64;

// ---- the weight differences, formed in fp32 on the device: wd [3][P] = W_m[0] - W_m[1] for the W_a, W_b and W_c thirds
__global__ __launch_bounds__(256) void bank_weight_delta_kernel(const float* __restrict__ Wm, float* __restrict__ wd, int P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < 3 * P) wd[e] = Wm[e] - Wm[3 * P + e];
}

// ---- sa_n for rows [first, first + n): one wave per row
template <int P>
__global__ __launch_bounds__(256) void bank_row_term_kernel(const float* __restrict__ U, const float* __restrict__ wd, float* __restrict__ sa, long long first, long long n) {
  ks_row_term<P>(U, wd, sa, first, n);
}

// ---- one group of nq vectors v [nq][P] -> vT [P][Qs] (zeros behind nq) and bv [Qs]; one thread per slot
template <int P>
__global__ __launch_bounds__(64) void bank_vector_prep_kernel(const float* __restrict__ v, const float* __restrict__ wd, float* __restrict__ vT, float* __restrict__ bv, int nq, int Qs) {
  ks_vector_prep<P>(v, wd, vT, bv, nq, Qs);
}

struct BankMarkArgs {
  long long first, count;      // the rows in range; block b takes rows first + b BR ..
  long long nblocks, W;        // row blocks; words per vector = ceil(count / 64)
  int nq, Qs, q0;              // vectors of the group, its padded width (a multiple of BK_QT), and the group's first vector
  int same_idx;
  const float* thr;            // [Q], one per vector
  bk_u64* bits;                // the group's slice of B: [nq][W]
};

template <int P, int BR>
__global__ __launch_bounds__(BR) void bank_mark_kernel(const float* __restrict__ U, const float* __restrict__ sa, const float* __restrict__ vT,
                                                       const float* __restrict__ bv, const float* __restrict__ wd, BankMarkArgs a) {
  constexpr int NW = BR / 64, STRIDE = BK_MI + 4, NST = BK_MI / 4;  // NST float4 per thread per step (BR threads stage BR rows x BK_MI features)
  static_assert(BR % 64 == 0 && P % (2 * BK_MI) == 0, "tile");
  __shared__ __attribute__((aligned(16))) float sv[BR * STRIDE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // grid: x = tile of vectors (fastest), (y, z) = row block: the workgroups that read the same rows are dispatched next to each other
  const long long rb = blockIdx.y + (long long)blockIdx.z * BK_GRID_Y;
  if (rb >= a.nblocks) return;  // (the whole workgroup: the last z-slice is ragged)
  const long long r0 = rb * BR;
  const int t0 = blockIdx.x * BK_QT;  // first vector of the tile, within the group
  const long long widx = rb * NW + w; // this wave's word of the range
  const float* Ub = U + (size_t)a.first * P;
  bk_f4 stage[2][NST];
  // rows past the range read its last row (never claimed): a select on the address, not on the value (no branch around the loads)
#define BK_LOAD_CHUNK(ST, I0)                                                        \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (BK_MI / 4), c4 = e % (BK_MI / 4);           \
    const long long gr = r0 + r < a.count ? r0 + r : a.count - 1;                    \
    stage[ST][j] = *(const bk_f4*)(Ub + (size_t)gr * P + (I0) + 4 * c4);             \
  }
#define BK_STORE_CHUNK(ST)                                                           \
  _Pragma("unroll") for (int j = 0; j < NST; ++j) {                                  \
    const int e = tid + BR * j, r = e / (BK_MI / 4), c4 = e % (BK_MI / 4);           \
    *(bk_f4*)(sv + r * STRIDE + 4 * c4) = stage[ST][j];                              \
  }
  float dd[BK_QT];
#pragma unroll
  for (int j = 0; j < BK_QT; ++j) dd[j] = 0.f;
  const float* myrow = sv + tid * STRIDE;
  const float* wc = wd + 2 * P;
  const float* vt = vT + t0;
  // Left alone, hipcc pairs neighbouring chains into packed fp32 operations, which have no |x| source modifier and are no faster per value than the plain forms.
  // An EMPTY asm statement that names the sixteen values keeps them scalar; it emits no instruction of its own.
  static_assert(BK_QT == 16, "BK_OPAQUE16 names sixteen values");
#define BK_OPAQUE16(X)                                                                                                                   \
  asm("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]), "+v"(X[6]), "+v"(X[7]), "+v"(X[8]), "+v"(X[9]), \
           "+v"(X[10]), "+v"(X[11]), "+v"(X[12]), "+v"(X[13]), "+v"(X[14]), "+v"(X[15]));
  // one chunk: every lane walks its row's BK_MI features in ascending order; per feature the BK_QT vector values and the weight are wave-uniform
#define BK_COMPUTE(I0)                                                               \
  _Pragma("unroll 1") for (int q = 0; q < BK_MI / 4; ++q) {                          \
    const bk_f4 uu = *(const bk_f4*)(myrow + 4 * q);                                 \
    const float* vq = vt + (size_t)((I0) + 4 * q) * a.Qs;                            \
    const float* wq = wc + (I0) + 4 * q;                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
      const float wv = wq[e];                                                        \
      float t[BK_QT];                                                                \
      _Pragma("unroll") for (int j = 0; j < BK_QT; ++j) t[j] = uu[e] - vq[(size_t)e * a.Qs + j]; \
      BK_OPAQUE16(t)                                                                 \
      _Pragma("unroll") for (int j = 0; j < BK_QT; ++j) dd[j] = fmaf(wv, fabsf(t[j]), dd[j]);    \
      BK_OPAQUE16(dd)                                                                \
    }                                                                                \
  }
  BK_LOAD_CHUNK(0, 0)
  BK_LOAD_CHUNK(1, BK_MI)
#pragma unroll 1
  for (int i0 = 0; i0 < P; i0 += 2 * BK_MI) {  // two chunks per trip: `stage` keeps compile-time indices and stays in registers
    BK_STORE_CHUNK(0)
    __syncthreads();
    if (i0 + 2 * BK_MI < P) { BK_LOAD_CHUNK(0, i0 + 2 * BK_MI) }
    BK_COMPUTE(i0)
    __syncthreads();  // every wave is done with this chunk before the next one overwrites it
    BK_STORE_CHUNK(1)
    __syncthreads();
    if (i0 + 3 * BK_MI < P) { BK_LOAD_CHUNK(1, i0 + 3 * BK_MI) }
    BK_COMPUTE(i0 + BK_MI)
    __syncthreads();
  }
#undef BK_LOAD_CHUNK
#undef BK_STORE_CHUNK
#undef BK_COMPUTE
#undef BK_OPAQUE16
  // ---- softmax_2 of the class difference, as the matcher forms it; a lane past the range holds a NaN, which claims nothing
  const long long rr = r0 + tid;
  const bool live = rr < a.count;
  const float sar = sa[a.first + (live ? rr : a.count - 1)];
  float ps[BK_QT];
#pragma unroll
  for (int j = 0; j < BK_QT; ++j) {
    const float dl = (sar + bv[t0 + j]) + dd[j];
    const float ed = expf(-fabsf(dl));
    const float inv = 1.0f / (1.0f + ed);
    const float p0 = dl >= 0.f ? inv : ed * inv, p1 = dl >= 0.f ? ed * inv : inv;
    ps[j] = live ? (a.same_idx == 0 ? p0 : p1) : __builtin_nanf("");
  }
  int lo = 0, hi = 0;  // lane j: the wave's word of vector t0 + j
#pragma unroll
  for (int j = 0; j < BK_QT; ++j) {
    const int q = a.q0 + t0 + (t0 + j < a.nq ? j : 0);  // (a padded slot reads a threshold that exists; its word is not stored)
    const bk_u64 word = __ballot(ps[j] >= a.thr[q]);
    lo = lane == j ? (int)(unsigned)word : lo;
    hi = lane == j ? (int)(unsigned)(word >> 32) : hi;
  }
  if (lane < BK_QT && t0 + lane < a.nq && widx < a.W) a.bits[(size_t)(t0 + lane) * a.W + widx] = ((bk_u64)(unsigned)hi << 32) | (unsigned)lo;
}

// ---- posword [W]: bit l of word w = row first + 64 w + l is of class 1; lanes past the range contribute nothing.  One wave per word.
__global__ __launch_bounds__(256) void bank_class_words_kernel(const uint8_t* __restrict__ cls, bk_u64* __restrict__ pos, long long first, long long count, long long W) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= W) return;  // (a whole wave)
  const long long r = w * 64 + lane;
  const bk_u64 word = __ballot(r < count && cls[first + (r < count ? r : 0)] != 0);
  if (lane == 0) pos[w] = word;
}

// ---- claimed [Q][2]: one workgroup per vector
__global__ __launch_bounds__(256) void bank_totals_kernel(const bk_u64* __restrict__ bits, const bk_u64* __restrict__ pos, long long* __restrict__ claimed, long long W) {
  __shared__ long long s0[256], s1[256];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  long long c0 = 0, c1 = 0;
  for (long long i = tid; i < W; i += 256) {
    const bk_u64 b = bits[q * W + i], p = pos[i];
    c1 += __popcll(b & p);
    c0 += __popcll(b & ~p);
  }
  s0[tid] = c0;
  s1[tid] = c1;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (tid < step) {
      s0[tid] += s0[tid + step];
      s1[tid] += s1[tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    claimed[2 * q] = s0[0];
    claimed[2 * q + 1] = s1[0];
  }
}

// ---- multiplicity: hist [2][Q + 1], sole [Q][2] (both zeroed by the caller, added to by integer atomics), mult [count] and sole_of [count] (either may be NULL)
__global__ __launch_bounds__(256) void bank_multiplicity_kernel(const bk_u64* __restrict__ bits, const bk_u64* __restrict__ pos, int Q, long long W, long long count,
                                                                int chunk, bk_u64* __restrict__ hist, bk_u64* __restrict__ sole,
                                                                uint16_t* __restrict__ mult, int32_t* __restrict__ sole_of) {
  __shared__ unsigned int lh[2 * (BK_QMAX + 1)], ls[2 * BK_QMAX];  // this workgroup's histogram [2][Q + 1] and sole counts [Q][2]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < 2 * (Q + 1); i += 256) lh[i] = 0u;
  for (int i = tid; i < 2 * Q; i += 256) ls[i] = 0u;
  __syncthreads();
  const long long w0 = (long long)blockIdx.x * chunk;
  for (int k = wv; k < chunk; k += 4) {  // (wave-uniform bounds)
    const long long w = w0 + k;
    if (w >= W) break;
    int m = 0, who = -1;
    const bk_u64* col = bits + w;
    for (int q = 0; q < Q; ++q) {
      const bk_u64 word = col[(size_t)q * W];  // (the same address in every lane)
      const int bit = (int)((word >> lane) & 1ull);
      m += bit;
      who = bit ? q : who;
    }
    const long long r = w * 64 + lane;
    if (r < count) {  // lanes past the range are rows that do not exist: not in hist[.][0] either
      const int c = (int)((pos[w] >> lane) & 1ull);
      atomicAdd(&lh[c * (Q + 1) + m], 1u);
      if (m == 1) atomicAdd(&ls[2 * who + c], 1u);
      if (mult) mult[r] = (uint16_t)m;
      if (sole_of) sole_of[r] = m == 1 ? who : -1;
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * (Q + 1); i += 256)
    if (lh[i]) atomicAdd(&hist[i], (bk_u64)lh[i]);
  for (int i = tid; i < 2 * Q; i += 256)
    if (ls[i]) atomicAdd(&sole[i], (bk_u64)ls[i]);
}

// ---- overlap [Q][Q][2] (zeroed by the caller): workgroup (x = tile pair of the upper triangle, y = word chunk of `chunk` words)
__global__ __launch_bounds__(256) void bank_overlap_kernel(const bk_u64* __restrict__ bits, const bk_u64* __restrict__ pos, int Q, long long W, int chunk,
                                                           const int* __restrict__ tiles /* [pairs][2] */, bk_u64* __restrict__ overlap) {
  constexpr int STR = BK_OW + 1;  // (the lanes of a wave read 32 different rows of tb at one word: an odd row stride spreads them over the banks)
  __shared__ bk_u64 ta[BK_OT * STR], tb[BK_OT * STR], tp[BK_OW];
  const int tid = threadIdx.x;
  const int qa = tiles[2 * blockIdx.x] * BK_OT, qb = tiles[2 * blockIdx.x + 1] * BK_OT;
  const bool diag = qa == qb;
  const long long w0 = (long long)blockIdx.y * chunk;
  const long long w1 = w0 + chunk < W ? w0 + chunk : W;
  const int j = tid & 31, i0 = tid >> 5;  // this thread's pairs: (qa + i0 + 8 k, qb + j), k = 0 .. 3
  int n[4] = {0, 0, 0, 0}, n1[4] = {0, 0, 0, 0};  // (a workgroup covers at most 2^31 - 1 rows: the caller bounds `chunk`)
  for (long long ws = w0; ws < w1; ws += BK_OW) {
    const int nw = (int)(w1 - ws < BK_OW ? w1 - ws : BK_OW);
    __syncthreads();  // (the last step's readers are done)
    for (int e = tid; e < BK_OT * BK_OW; e += 256) {
      const int r = e / BK_OW, c = e % BK_OW;
      ta[r * STR + c] = (qa + r < Q && c < nw) ? bits[(size_t)(qa + r) * W + ws + c] : 0ull;
      tb[r * STR + c] = (qb + r < Q && c < nw) ? bits[(size_t)(qb + r) * W + ws + c] : 0ull;
    }
    if (tid < BK_OW) tp[tid] = tid < nw ? pos[ws + tid] : 0ull;
    __syncthreads();
    for (int c = 0; c < nw; ++c) {
      const bk_u64 b = tb[j * STR + c], p = tp[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bk_u64 x = ta[(i0 + 8 * k) * STR + c] & b;
        n[k] += __popcll(x);
        n1[k] += __popcll(x & p);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = qa + i0 + 8 * k, r = qb + j;
    if (q < Q && r < Q && (!diag || q <= r) && n[k]) {
      bk_u64* o = overlap + ((size_t)q * Q + r) * 2;
      if (n[k] - n1[k]) atomicAdd(o, (bk_u64)(n[k] - n1[k]));
      if (n1[k]) atomicAdd(o + 1, (bk_u64)n1[k]);
    }
  }
}

// ---- the upper triangle copied below the diagonal: a launch of its own
__global__ __launch_bounds__(256) void bank_mirror_kernel(bk_u64* __restrict__ overlap, int Q) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)Q * Q) return;
  const int q = (int)(e / Q), r = (int)(e % Q);
  if (r < q) {
    overlap[((size_t)q * Q + r) * 2] = overlap[((size_t)r * Q + q) * 2];
    overlap[((size_t)q * Q + r) * 2 + 1] = overlap[((size_t)r * Q + q) * 2 + 1];
  }
}

struct BankGreedyState {  // one per index, on the device
  int rounds, done;
};

// ---- the start of a greedy cover: taken [Q] = fixed != 0; covered [W] = OR of the fixed vectors' rows: one thread per word
__global__ __launch_bounds__(256) void bank_cover_init_kernel(const bk_u64* __restrict__ bits, const uint8_t* __restrict__ taken, int Q, long long W,
                                                              bk_u64* __restrict__ covered, BankGreedyState* __restrict__ st) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w == 0) {
    st->rounds = 0;
    st->done = 0;
  }
  if (w >= W) return;
  bk_u64 c = 0ull;
  for (int q = 0; q < Q; ++q)
    if (taken[q]) c |= bits[(size_t)q * W + w];
  covered[w] = c;
}

// ---- partials [Q][nchunks][2] = (newneg, newpos) of vector q over chunk y
__global__ __launch_bounds__(256) void bank_gain_kernel(const bk_u64* __restrict__ bits, const bk_u64* __restrict__ pos, const bk_u64* __restrict__ covered,
                                                        const uint8_t* __restrict__ taken, long long W, int chunk, int nchunks,
                                                        const BankGreedyState* __restrict__ st, long long* __restrict__ part) {
  __shared__ int s0[256], s1[256];
  if (st->done) return;  // (written by an EARLIER launch)
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  if (taken[q]) return;  // (fixed, or picked in an earlier round: the pick kernel does not read its partials)
  const long long w0 = (long long)blockIdx.y * chunk;
  const long long w1 = w0 + chunk < W ? w0 + chunk : W;
  int c0 = 0, c1 = 0;  // (a chunk holds fewer than 2^31 rows: the caller bounds it)
  for (long long i = w0 + tid; i < w1; i += 256) {
    const bk_u64 b = bits[q * W + i] & ~covered[i], p = pos[i];
    c1 += __popcll(b & p);
    c0 += __popcll(b & ~p);
  }
  s0[tid] = c0;
  s1[tid] = c1;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (tid < step) {
      s0[tid] += s0[tid + step];
      s1[tid] += s1[tid + step];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[(q * nchunks + blockIdx.y) * 2] = s0[0];
    part[(q * nchunks + blockIdx.y) * 2 + 1] = s1[0];
  }
}

// ---- one workgroup: the round's pick
__global__ __launch_bounds__(BK_PICK_THREADS) void bank_pick_kernel(const bk_u64* __restrict__ bits, bk_u64* __restrict__ covered, uint8_t* __restrict__ taken, int Q,
                                                                    long long W, int nchunks, const long long* __restrict__ part, long long w_pos, long long w_neg,
                                                                    int max_rounds, BankGreedyState* __restrict__ st, int32_t* __restrict__ order,
                                                                    long long* __restrict__ gained) {
  __shared__ long long sg[BK_PICK_THREADS], sp[BK_PICK_THREADS], sn[BK_PICK_THREADS];
  __shared__ int sq[BK_PICK_THREADS];
  if (st->done) return;
  const int tid = threadIdx.x;
  const int round = st->rounds;
  long long bg = 0, bp = 0, bn = 0;
  int bq = -1;  // (no candidate)
  for (int q = tid; q < Q; q += BK_PICK_THREADS) {  // ascending q per thread: a later equal gain does not replace an earlier one
    if (taken[q]) continue;
    long long n0 = 0, n1 = 0;
    for (int c = 0; c < nchunks; ++c) {
      n0 += part[((size_t)q * nchunks + c) * 2];
      n1 += part[((size_t)q * nchunks + c) * 2 + 1];
    }
    const long long g = w_pos * n1 - w_neg * n0;
    if (bq < 0 || g > bg) {
      bg = g; bp = n1; bn = n0; bq = q;
    }
  }
  sg[tid] = bg; sp[tid] = bp; sn[tid] = bn; sq[tid] = bq;
  __syncthreads();
  for (int step = BK_PICK_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) {
      const int oq = sq[tid + step];
      const long long og = sg[tid + step];
      const int mq = sq[tid];
      // the other side wins when this side has no candidate, or its gain is higher, or equal with the lower index
      if (oq >= 0 && (mq < 0 || og > sg[tid] || (og == sg[tid] && oq < mq))) {
        sg[tid] = og; sp[tid] = sp[tid + step]; sn[tid] = sn[tid + step]; sq[tid] = oq;
      }
    }
    __syncthreads();
  }
  const int q = sq[0];
  const bool pick = q >= 0 && sg[0] > 0 && round < max_rounds;  // (the same in every thread)
  if (!pick) {
    if (tid == 0) st->done = 1;
    return;
  }
  for (long long i = tid; i < W; i += BK_PICK_THREADS) covered[i] |= bits[(size_t)q * W + i];
  if (tid == 0) {
    order[round] = q;
    gained[2 * round] = sp[0];
    gained[2 * round + 1] = sn[0];
    taken[q] = 1;
    st->rounds = round + 1;
  }
}
