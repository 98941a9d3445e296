// Compute dtype MV_F32, the reference form: the encoder in fp32 on the fp32-input matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products,
// fp32 accumulation, bitwise an fmaf chain; 1/16 of the 16-bit matrix rate).  The arithmetic the reference runs, inside the library, for audits
// and envelope work (memvul_amd/audit.py) — not for throughput.  Two kernels: the GEMM of all four projections and the attention.  Embedding,
// LayerNorm, pooler, header, matcher: the fp32 kernels of misc_kernels.h / match_topk.h, unchanged.
#pragma once
#include "common.h"

// ---- C[M][N] = act(A[M][K] W[N][K]^T + bias) (+ res) --------------------------------------------------------------------------------------
// Both operands "rows of K" in fp32 (torch Linear.weight layout).  A workgroup of four waves owns one 128 x 128 output tile and the WHOLE K of
// it, in tiles of 32; a wave owns 64 x 64 of it as 2 x 2 fragments of 32 x 32 — four independent accumulators, which is what keeps the matrix
// pipe issuing (the instruction's dependent-accumulator latency equals its issue time).
// Order of summation: the instruction contracts two k per issue, lanes 0 - 31 supplying one and lanes 32 - 63 the other.  Which two is free as
// long as A and B agree, so lanes 0 - 31 walk k = 0 .. 15 of a K-tile and lanes 32 - 63 k = 16 .. 31: issue t adds (k0 + t, k0 + 16 + t) —
// a lane then reads 16 CONSECUTIVE floats of its row from LDS (four 16-byte reads) instead of 16 strided dwords.  Every K-tile is summed into an accumulator
// of its own (16 issues from zero) and the tile sums are added up in ascending order — blocked summation, as the CPU libraries the reference runs on do it: ONE
// chain over the whole K rounds every step at the magnitude of the full partial sum and read up to 2.6 g(K) sum |a b| on random operands (g = the chain's
// 1.5e-7 at K = 768), above the 2 g the GEMM test allows; in blocks only K / 32 additions happen at that magnitude.  The order is fixed by (K)
// alone: a row's bits depend on nothing but the row and the weights (not on M, the tile it lands in, or the batch around it).
// LDS: rows of 32 floats at a pitch of 36 (144 B: 16-byte aligned, and 36 i mod 64 for i = 0 .. 15 hits 16 distinct multiples of 4, so the 16
// lanes a 16-byte read serves per cycle cover the 64 banks once: no bank conflict; a pitch of 32 would be a 32-way one).
// Pipeline: the next K-tile's global loads (8 x 16 B per thread) are issued before the current tile's 64 MFMAs and stored to LDS after them.
// Requires M % 128 == 0, N % 128 == 0, K % 32 == 0 (the engine's passes: M % 256, N in {768, 2304, 3072}, K in {768, 3072}).
// `res` may alias C (the residual stream in place): every element is read and written by the same thread.
#define RF_ACT_NONE 0  // bias only (QKV)
#define RF_ACT_GELU 1  // exact-erf GELU (FFN-1)
#define RF_ACT_RES 2   // bias + residual (attention output projection, FFN-2)
#define RF_PITCH 36

// erf-form GELU as the reference spells it (HF "gelu": x * 0.5 * (1 + erf(x / sqrt(2)))) on the device library's erff (about 1 ulp).  The 16-bit paths'
// gelu_erf (common.h) is a one-transcendental fit good to 7e-7 absolute: three orders below an fp16 rounding, but ten fp32 roundings — too coarse for the
// form every other form is measured against.
__device__ __forceinline__ float rf_gelu(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

template <int ACT>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* res, float* C, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float sA[128 * RF_PITCH];
  __shared__ __attribute__((aligned(16))) float sB[128 * RF_PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tn = N / 128;
  const int m0 = (blockIdx.x / tn) * 128, n0 = (blockIdx.x % tn) * 128;  // neighbouring workgroups share their A rows
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int hi = lane >> 5, l31 = lane & 31;
  // staging: thread -> (row, 16-byte piece) of a 128 x 32 tile, four rows 32 apart per operand
  const int srow = tid >> 3, scol = (tid & 7) * 4;
  const float* gA = A + (size_t)(m0 + srow) * K + scol;
  const float* gB = W + (size_t)(n0 + srow) * K + scol;
  floatx4 ra[4], rb[4];  // (clang vectors: HIP's float4 struct, live across the K loop, ends up in scratch)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = *(const floatx4*)(gA + (size_t)(32 * i) * K);
    rb[i] = *(const floatx4*)(gB + (size_t)(32 * i) * K);
  }
  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int nk = K / 32;
#pragma unroll 1
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(floatx4*)(sA + (srow + 32 * i) * RF_PITCH + scol) = ra[i];
      *(floatx4*)(sB + (srow + 32 * i) * RF_PITCH + scol) = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = *(const floatx4*)(gA + (size_t)(32 * i) * K + 32 * (kt + 1));
        rb[i] = *(const floatx4*)(gB + (size_t)(32 * i) * K + 32 * (kt + 1));
      }
    }
    floatx4 fa[2][4], fb[2][4];  // this lane's 16 k of rows wm + 32 i + l31 / columns wn + 32 j + l31
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        fa[i][q] = *(const floatx4*)(sA + (wm + 32 * i + l31) * RF_PITCH + 16 * hi + 4 * q);
        fb[i][q] = *(const floatx4*)(sB + (wn + 32 * i + l31) * RF_PITCH + 16 * hi + 4 * q);
      }
    floatx16 blk[2][2];  // this K-tile's own sum (see "Order of summation")
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) blk[i][j][r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#define RF_STEP(c)                                                                               \
      blk[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0][q].c, fb[0][q].c, blk[0][0], 0, 0, 0); \
      blk[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0][q].c, fb[1][q].c, blk[0][1], 0, 0, 0); \
      blk[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1][q].c, fb[0][q].c, blk[1][0], 0, 0, 0); \
      blk[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1][q].c, fb[1][q].c, blk[1][1], 0, 0, 0)
      RF_STEP(x); RF_STEP(y); RF_STEP(z); RF_STEP(w);
#undef RF_STEP
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] += blk[i][j];
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn + 32 * j + l31;
    const float b = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const size_t o = (size_t)(m0 + wm + 32 * i + mfma32_row(r, hi)) * N + col;
        float v = acc[i][j][r] + b;
        if constexpr (ACT == RF_ACT_GELU) v = rf_gelu(v);
        else if constexpr (ACT == RF_ACT_RES) v += res[o];
        C[o] = v;
      }
  }
}

// ---- attention in fp32 --------------------------------------------------------------------------------------------------------------------
// qkv [B Sp][2304]: the QKV projection's output, Q (with the folded 1/8) | K | V, head h in columns 64 h .. 64 h + 63 of each block.  ctx [B Sp][768].
// One wave owns 32 queries of one (sequence, head) and walks the keys in chunks of 32, twice, with nothing in LDS:
//   pass 1: S^T = K Q^T chunk by chunk (keys = rows of the C fragment, i.e. registers; queries = its columns, i.e. lanes), the running maximum and the
//           running sum of exp(s - max) per query;
//   pass 2: S^T again, p = exp(s - max) / sum — the softmax as the reference forms it, normalised BEFORE P V — and O += P V with the S^T fragment as the A
//           operand as it stands: register r of a lane holds key (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of query lane & 31, which is A[i = query][k = key]
//           of an issue that contracts keys (kr, kr + 4): the B operand is V[kr + 4 (lane >> 5)][d = lane & 31], read straight from the row-major V.
// Recomputing S costs a quarter more of 5 - 10 % of the FLOPs and spares the rescaling of O (whose rows are registers while the factors live in lanes).
// The contraction over d uses the same freedom as the GEMM: lanes 0 - 31 carry d = 0 .. 31, lanes 32 - 63 d = 32 .. 63 (a lane reads 128 consecutive bytes).
// Keys j >= len are left out — what the reference's additive -10000 gives in fp32 (exp underflows to exactly 0) — chunks past len are never visited.
// Query rows >= len are computed like any other (the reference does; nobody reads them).  Everything is per (sequence, head, query): a row's bits do not
// depend on the batch.
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lens, float* __restrict__ ctx,
                                                            int Sp, int units) {
  const int lane = threadIdx.x & 63, hi = lane >> 5, l31 = lane & 31;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);  // (sequence, head, 32-query block); wave-uniform
  if (unit >= units) return;
  const int nqb = Sp / 32;
  const int qb = unit % nqb, bh = unit / nqb, h = bh % MV_HEADS, b = bh / MV_HEADS;
  int len = lens[b];
  len = len < 1 ? 1 : (len > Sp ? Sp : len);
  const int nch = (len + 31) / 32;
  constexpr int LD = 3 * MV_HIDDEN;
  const float* base = qkv + (size_t)b * Sp * LD + h * MV_HEAD_DIM;
  float4 q4[8];  // Q[query l31][d = 32 hi .. 32 hi + 31]
  {
    const float* qp = base + (size_t)(qb * 32 + l31) * LD + 32 * hi;
#pragma unroll
    for (int i = 0; i < 8; ++i) q4[i] = *(const float4*)(qp + 4 * i);
  }
  auto scores = [&](int c) -> floatx16 {  // S^T of chunk c: register r = key 32 c + mfma32_row(r, hi), query l31; masked keys = -inf
    const float* kp = base + MV_HIDDEN + (size_t)(c * 32 + l31) * LD + 32 * hi;
    float4 k4[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k4[i] = *(const float4*)(kp + 4 * i);
    floatx16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4[i].x, q4[i].x, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4[i].y, q4[i].y, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4[i].z, q4[i].z, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4[i].w, q4[i].w, s, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (c * 32 + mfma32_row(r, hi) >= len) s[r] = -INFINITY;
    return s;
  };
  // pass 1: per lane over its 16 keys of every chunk, then the two halves of the wave (the other 16 keys of each chunk) combined
  float m = -INFINITY, l = 0.f;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const floatx16 s = scores(c);
    float cm = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) cm = fmaxf(cm, s[r]);
    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));  // key 32 c is never masked (c < nch): finite from here on
    const float mn = fmaxf(m, cm);
    float a = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) a += expf(s[r] - mn);
    a += __shfl_xor(a, 32, 64);
    l = l * expf(m - mn) + a;  // (first chunk: l = 0, exp(-inf) = 0)
    m = mn;
  }
  const float inv = 1.0f / l;
  // pass 2
  floatx16 o0, o1;  // O[query mfma32_row(r, hi)][d = l31] and [d = 32 + l31]
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const floatx16 s = scores(c);
    const float* vp = base + 2 * MV_HIDDEN + (size_t)(c * 32 + 4 * hi) * LD + l31;
    float v0[16], v1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = (r & 3) + 8 * (r >> 2);
      v0[r] = vp[(size_t)kr * LD];
      v1[r] = vp[(size_t)kr * LD + 32];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = expf(s[r] - m) * inv;
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(p, v0[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(p, v1[r], o1, 0, 0, 0);
    }
  }
  float* op = ctx + (size_t)(b * Sp + qb * 32) * MV_HIDDEN + h * MV_HEAD_DIM + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    op[(size_t)mfma32_row(r, hi) * MV_HIDDEN] = o0[r];
    op[(size_t)mfma32_row(r, hi) * MV_HIDDEN + 32] = o1[r];
  }
}
