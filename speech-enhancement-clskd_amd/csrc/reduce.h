// Fixed-order fp64 block reductions shared by the normalisation, loss and metric kernels (device
// code only).  A helper's summation order is part of its contract: the callers' results are
// bitwise repeatable and compared bit for bit across changes.
#pragma once
#include "common.h"

namespace clskd {

// T-thread tree: v[k] <- sum over the block's threads of v[k], valid in every thread.  Order:
// thread t adds thread t + o's value for o = T/2, T/4, ..., 1 (one barrier per level, the NQ
// quantities side by side).  LDS: NQ * T doubles per <NQ, T>; two calls of one <NQ, T> in a
// kernel need a barrier between them (the second call's stores against the first call's reads).
template <int NQ, int T = 256>
__device__ __forceinline__ void block_tree_sum(double (&v)[NQ]) {
  __shared__ double red[NQ][T];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NQ; ++k) red[k][tid] = v[k];
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < NQ; ++k) red[k][tid] += red[k][tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) v[k] = red[k][0];
}

template <int T = 256>
__device__ __forceinline__ double block_tree_sum(double v) {
  double a[1] = {v};
  block_tree_sum<1, T>(a);
  return a[0];
}

// Row-lane block sum of a 256-thread block whose thread tid = rl * CG + cg holds, in each array of
// `acc` (double[4], one array per quantity k = 0 .. NQ - 1), the sums of channels cg * 4 + j over
// the rows of row lane rl (CG = C / 4 quads per row, RP = 256 / CG row lanes; a thread with
// rl >= RP passes zeros, which are never read).  Block blockIdx.x's row of the partial table gets
//   partial[(blockIdx.x * C + cg * 4 + j) * STRIDE + k] = sum over l = 0 .. RP - 1, ascending,
// of lane l's value, by the quad's first thread in a single level; entries k in [NQ, STRIDE) are
// written as 0.0.  LDS: red[256][4 * NQ + 1] (odd stride).
// The accumulators and the totals are one array per quantity on purpose: the compiler keeps such
// an array as one 4-vector, and one [NQ][4] array instead gave BatchNorm's backward reduce
// another register assignment (85 VGPRs against 81, profiles/bn_core_codegen.txt).
template <int STRIDE, typename... Acc>
__device__ __forceinline__ void row_lane_block_sum(int C, double* __restrict__ partial,
                                                   const Acc&... acc) {
  constexpr int NQ = sizeof...(Acc);
  static_assert(NQ >= 1 && STRIDE >= NQ, "a partial row holds every quantity");
  __shared__ double red[256][4 * NQ + 1];
  const int CG = C >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int k = 0;
    ((red[tid][4 * k++ + j] = acc[j]), ...);  // quantity k at red[tid][4 * k + j]
  }
  __syncthreads();
  if (tid < CG) {
    static_assert(NQ <= 3, "one array of totals per quantity");
    double t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
    for (int l = 0; l < RP; ++l) {
      const int t = l * CG + tid;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        t0[j] += red[t][j];
        if constexpr (NQ > 1) t1[j] += red[t][4 + j];
        if constexpr (NQ > 2) t2[j] += red[t][8 + j];
      }
    }
    double* p = partial + ((int64_t)blockIdx.x * C + tid * 4) * STRIDE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p[STRIDE * j] = t0[j];
      if constexpr (NQ > 1) p[STRIDE * j + 1] = t1[j];
      if constexpr (NQ > 2) p[STRIDE * j + 2] = t2[j];
#pragma unroll
      for (int k = NQ; k < STRIDE; ++k) p[STRIDE * j + k] = 0.0;
    }
  }
}

// The two-level form (ComplexBatchNorm), acc[k][j] holding quantity k and `out` being the block's
// row of the partial table (STRIDE = NQ):
// G = min(16, RP) groups — group g sums lanes g, g + G, ... in that order, one thread per group
// and quad — and then the quad's first thread sums the groups 0 .. G - 1.  With one quad per row
// (C = 8) the single level leaves one thread walking 256 LDS rows per pass.  Two quantities per
// LDS pass (red[256][9]).  A different order from row_lane_block_sum: not interchangeable.
template <int NQ>
__device__ __forceinline__ void row_lane_block_sum_2level(const double (&acc)[NQ][4], int CG,
                                                          int RP, double* __restrict__ out) {
  __shared__ double red[256][9];
  const int tid = threadIdx.x;
  const int G = RP < 16 ? RP : 16;
  const int g = tid / CG, cgi = tid - g * CG;  // level-1 role of this thread (g < G)
#pragma unroll
  for (int k0 = 0; k0 < NQ; k0 += 2) {
    const int k1 = k0 + 1 < NQ ? k0 + 1 : k0;  // odd NQ: the last pass carries one quantity
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      red[tid][j] = acc[k0][j];
      red[tid][4 + j] = acc[k1][j];
    }
    __syncthreads();
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (g < G) {
      for (int l = g; l < RP; l += G) {
        const int t = l * CG + cgi;
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += red[t][j];
      }
    }
    __syncthreads();
    if (g < G) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[tid][j] = a[j];  // row g * CG + cgi = tid
    }
    __syncthreads();
    if (tid < CG) {
      double b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int l = 0; l < G; ++l) {
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] += red[l * CG + tid][j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[(tid * 4 + j) * NQ + k0] = b[j];
        if (k0 + 1 < NQ) out[(tid * 4 + j) * NQ + k0 + 1] = b[4 + j];
      }
    }
    __syncthreads();
  }
}

// Per-channel sum of a partial table (one 256-thread block per channel c):
//   tot[k] = sum over b < nblk of partial[(b * C + c) * NQ + k], valid in every thread.
// Order: thread t sums rows t, t + 256, ... ascending — with U > 1, while U rows U * 256 apart
// remain, row t + u * 256 goes to accumulator u (U loads in flight per thread), the rest to
// accumulator 0, and the accumulators combine pairwise, ((0+1)+(2+3))+((4+5)+(6+7)) for U = 8 —
// then block_tree_sum over the threads.  The U-wide loop is entered only when
// nblk > (U - 1) * 256; below that every U gives the bits of U = 1 (the combine adds exact
// zeros, and an accumulator that starts at +0.0 never holds -0.0).
template <int NQ, int U>
__device__ __forceinline__ void channel_partial_sum(const double* __restrict__ partial, int nblk,
                                                    int C, int c, double (&tot)[NQ]) {
  static_assert(U >= 1 && (U & (U - 1)) == 0, "pairwise combine: U a power of two");
  double s[U][NQ];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < NQ; ++k) s[u][k] = 0.0;
  int b = threadIdx.x;
  if constexpr (U > 1) {
    for (; b + (U - 1) * 256 < nblk; b += U * 256) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double* p = partial + ((int64_t)(b + u * 256) * C + c) * NQ;
#pragma unroll
        for (int k = 0; k < NQ; ++k) s[u][k] += p[k];
      }
    }
  }
  for (; b < nblk; b += 256) {
    const double* p = partial + ((int64_t)b * C + c) * NQ;
#pragma unroll
    for (int k = 0; k < NQ; ++k) s[0][k] += p[k];
  }
#pragma unroll
  for (int w = 1; w < U; w *= 2)
#pragma unroll
    for (int u = 0; u < U; u += 2 * w)
#pragma unroll
      for (int k = 0; k < NQ; ++k) s[u][k] += s[u + w][k];
#pragma unroll
  for (int k = 0; k < NQ; ++k) tot[k] = s[0][k];
  block_tree_sum<NQ>(tot);
}

}  // namespace clskd
