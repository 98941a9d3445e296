// The per-row and per-vector terms of P(same) over a kept corpus, stated once for the kernel headers of the four kept-corpus libraries (per-anchor retrieval,
// per-anchor claims, the anchor-bank audit, per-anchor ranking quality).
//
// P(same)[n, g] is defined bit for bit: it is the fp32 value the engine's matcher (match_topk.h) produces for the pair (row n, vector g).  That value depends on the
// pair alone, so its arithmetic is restated here (NOT included: match_topk.h's inline launchers would instantiate the engine's kernels into these libraries):
//   sa_n    = sum (W_a[0] - W_a[1]) . u_n   lane l takes features l + 64 j by fmaf, j ascending from 0; then the six-step DPP ladder of ks_wave_sum
//   bv_g    = fma chain of (W_b[0] - W_b[1])[i] * v_g[i],           i ascending, from 0
//   dd_{n,g} = fma chain of (W_c[0] - W_c[1])[i] * |u_n[i] - v_g[i]|, i ascending, from 0      (the weight differences are formed in fp32 first)
//   delta = (sa_n + bv_g) + dd;  e = expf(-|delta|);  inv = 1 / (1 + e);  P_0 = delta >= 0 ? inv : e inv;  P_1 the other;  P(same) = P_{same_idx}
// sa_n and bv_g are formed by the functions below; dd and the ending belong to each library's score / mark kernel, which is tuned instruction by instruction and
// stays in its own header.  Every function here is inlined into a __global__ kernel of the including header, under that kernel's name: the libraries share text,
// not symbols.
#pragma once
#include <hip/hip_runtime.h>

// Wave-wide sum, the ladder of match_topk.h mk_wave_sum: row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31, lane 63 read
__device__ __forceinline__ float ks_wave_sum(float x) {
#define KS_SUM_STEP(CTRL, ROWS) x += __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), CTRL, ROWS, 0xf, false));
  KS_SUM_STEP(0x111, 0xf)
  KS_SUM_STEP(0x112, 0xf)
  KS_SUM_STEP(0x114, 0xf)
  KS_SUM_STEP(0x118, 0xf)
  KS_SUM_STEP(0x142, 0xa)
  KS_SUM_STEP(0x143, 0xc)
#undef KS_SUM_STEP
  return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(x), 63));
}

// ---- sa_n for rows [first, first + n): one wave per row, four rows per workgroup of 256
template <int P>
__device__ __forceinline__ void ks_row_term(const float* __restrict__ U, const float* __restrict__ wd, float* __restrict__ sa, long long first, long long n) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float* u = U + (size_t)(first + r) * P;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < P / 64; ++j) s = fmaf(wd[lane + 64 * j], u[lane + 64 * j], s);
  s = ks_wave_sum(s);
  if (lane == 0) sa[first + r] = s;
}

// ---- one group of nq vectors v [nq][P] -> vT [P][Qs] (zeros behind nq) and bv [Qs]; one thread per slot, workgroups of 64
template <int P>
__device__ __forceinline__ void ks_vector_prep(const float* __restrict__ v, const float* __restrict__ wd, float* __restrict__ vT, float* __restrict__ bv, int nq, int Qs) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= Qs) return;
  float s = 0.f;
  for (int i = 0; i < P; ++i) {
    const float x = q < nq ? v[(size_t)q * P + i] : 0.f;
    s = fmaf(wd[P + i], x, s);
    vT[(size_t)i * Qs + q] = x;
  }
  bv[q] = s;
}
