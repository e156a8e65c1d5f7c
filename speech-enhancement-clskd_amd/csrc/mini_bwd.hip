// Backward kernels of the asteroid DCCRNet_mini training step that have no counterpart in the
// local-DCCRN backward (norm_bwd.hip): the bounded complex mask times the spectrum and the
// output-level MSE distillation loss.  (The OnReIm BatchNorm + PReLU pair, one slope per part,
// is clskd_bn_bwd_reim beside clskd_bn_bwd in norm_bwd.hip: the same kernels with a switch.)
// HBM-bound passes; every reduction is fp64 partials combined in a fixed order (reduce.h; no
// float atomics, no agent-scope fences), so gradients and losses are bitwise repeatable.
#include <algorithm>

#include "common.h"
#include "reduce.h"

namespace clskd {

// ------------------------------------------------------------------------------------------
// BoundComplexMask('tanh') * spectrum backward (reverse of mask_bdt_kernel, norm.hip).
// Forward: bound = tanh(r) u with M = mr + i mi, r = |M|, u = M / r; est = bound * X on bins
// 0..255.  Given dest = dL/d est (re at f, im at 257 + f):
//   g = dL/d bound = conj(X) dest
//   dL/dM = (1 - s^2)(u.g) u + (s / r)(g - (u.g) u),  s = tanh r  (u, g as 2-vectors)
// At r = 0 the Jacobian's limit is the identity: dL/dM = g (the forward yields 0 there).
// The tiling of mask_e_bwd_kernel: MASK_TT frames per block, the mask columns staged in LDS and
// the gradient written back through the same tile in runs of 2 * nt floats per bin.  The padded
// row MASK_LD = 34 dwords keeps the compute loop's 8-byte reads (bank = dword % 64 per 32-lane
// half: bins 2k at dwords 4k, 4k + 1, bins 2k + 1 at 4k + 34, 4k + 35 mod 64) and the 4-byte tile
// loads / stores (32 consecutive dwords per half) conflict-free.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_bdt_bwd_kernel(
    const float* __restrict__ spec, int ldspec, const float* __restrict__ mask, int Tm, int B,
    int T, const float* __restrict__ dest, int ldest, float* __restrict__ dmask) {
  __shared__ __attribute__((aligned(16))) float ml[256 * MASK_LD];
  const int b = blockIdx.y, t0 = blockIdx.x * MASK_TT;
  const int nt = min(MASK_TT, T - t0);
  const int64_t col0 = ((int64_t)b * 256 * Tm + t0) * 2;
  mask_tile_load(mask + col0, Tm, nt, ml);
  __syncthreads();
  for (int i = threadIdx.x; i < nt * 256; i += 256) {
    const int tt = i >> 8, f = i & 255;
    const int64_t bt = (int64_t)b * T + t0 + tt;
    const float xr = spec[bt * ldspec + f], xi = spec[bt * ldspec + 257 + f];
    const float dre = dest[bt * ldest + f], dim = dest[bt * ldest + 257 + f];
    const float gr = xr * dre + xi * dim;
    const float gi = xr * dim - xi * dre;
    float* mp = ml + f * MASK_LD + 2 * tt;  // read, then overwritten by this thread only
    const float mr = mp[0], mi = mp[1];
    const float r = hypotf(mr, mi);
    float o0 = gr, o1 = gi;
    if (r > 0.f) {
      const float ur = mr / r, ui = mi / r;
      const float s = tanhf(r);
      const float ug = ur * gr + ui * gi;
      const float rad = (1.f - s * s) * ug;  // along u
      const float tan = s / r;               // across u
      o0 = rad * ur + tan * (gr - ug * ur);
      o1 = rad * ui + tan * (gi - ug * ui);
    }
    mp[0] = o0;
    mp[1] = o1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * 2 * MASK_TT; i += 256) {
    const int fm = i / (2 * MASK_TT), r = i - fm * 2 * MASK_TT;
    if (r < 2 * nt) dmask[col0 + (int64_t)fm * Tm * 2 + r] = ml[fm * MASK_LD + r];
  }
  if (blockIdx.x == 0 && Tm > T) {  // columns the forward never read: T <= tm < Tm
    const int nz = 2 * (Tm - T);
    for (int i = threadIdx.x; i < 256 * nz; i += 256) {
      const int fm = i / nz, j = i - fm * nz;
      dmask[(((int64_t)b * 256 + fm) * Tm + T) * 2 + j] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------
// F.mse_loss(a, b, 'mean') and its gradient in one pass: da (+)= gscale * (a - b) with gscale =
// scale * 2 / n, and one fp64 partial of sum (a - b)^2 per block.  VEC: 16-byte accesses (the
// three pointers 16-byte aligned), the n % 4 tail by the thread that would own the next quad.
// ------------------------------------------------------------------------------------------
constexpr int MSE_MAX_BLOCKS = 1024;

template <bool VEC>
__global__ __launch_bounds__(256) void mse_loss_grad_kernel(
    const float* __restrict__ a, const float* __restrict__ b, int64_t n, float gscale,
    float* __restrict__ da, int accumulate, double* __restrict__ partial) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double s = 0.0;
  if (VEC) {
    const int64_t nq = n >> 2;
    for (int64_t q = i0; q <= nq; q += stride) {
      if (q < nq) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + q * 4);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + q * 4);
        const f32x4 d = av - bv;
        f32x4 o = gscale * d;
        if (da) {
          if (accumulate) o += *reinterpret_cast<const f32x4*>(da + q * 4);
          *reinterpret_cast<f32x4*>(da + q * 4) = o;
        }
        s += ((double)d[0] * d[0] + (double)d[1] * d[1]) + ((double)d[2] * d[2] + (double)d[3] * d[3]);
      } else {
        for (int64_t i = nq * 4; i < n; ++i) {  // scalar tail
          const float d = a[i] - b[i];
          if (da) da[i] = accumulate ? da[i] + gscale * d : gscale * d;
          s += (double)d * d;
        }
      }
    }
  } else {
    for (int64_t i = i0; i < n; i += stride) {
      const float d = a[i] - b[i];
      if (da) da[i] = accumulate ? da[i] + gscale * d : gscale * d;
      s += (double)d * d;
    }
  }
  s = block_tree_sum(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// loss_out (+)= scale * (sum of the block partials, fixed order) / n
__global__ __launch_bounds__(256) void mse_loss_finalize_kernel(const double* __restrict__ partial,
                                                               int nblk, int64_t n, float scale,
                                                               float* loss_out, int accumulate) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  s = block_tree_sum(s);
  if (threadIdx.x == 0) {
    const float v = (float)((double)scale * s / (double)n);
    loss_out[0] = accumulate ? loss_out[0] + v : v;
  }
}

inline int mse_blocks(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(MSE_MAX_BLOCKS, cdiv(cdiv(n, 4) + 1, 256)));
}

}  // namespace clskd

using namespace clskd;

extern "C" int clskd_mask_bdt_bwd(const float* spec, int32_t ldspec, const float* mask, int32_t Tm,
                                  int32_t B, int32_t T, const float* dest, int32_t ldest,
                                  float* dmask, void* stream) {
  CLSKD_CHECK_ARG(spec && mask && dest && dmask, "mask_bdt_bwd: null pointer");
  CLSKD_CHECK_SHAPE(B > 0 && B <= 65535 && T > 0, "mask_bdt_bwd: B=%d T=%d", B, T);
  CLSKD_CHECK_SHAPE(Tm >= T, "mask_bdt_bwd: Tm=%d < T=%d", Tm, T);
  CLSKD_CHECK_SHAPE(ldspec >= 514 && ldest >= 514, "mask_bdt_bwd: ldspec=%d ldest=%d (< 514)",
                    ldspec, ldest);
  hipLaunchKernelGGL(mask_bdt_bwd_kernel, dim3((unsigned)cdiv(T, MASK_TT), (unsigned)B), dim3(256),
                     0, as_stream(stream), spec, ldspec, mask, Tm, B, T, dest, ldest, dmask);
  CLSKD_LAUNCH_CHECK("mask_bdt_bwd");
  return CLSKD_OK;
}

extern "C" int64_t clskd_mse_loss_grad_workspace(int64_t n) { return mse_blocks(n); }

extern "C" int clskd_mse_loss_grad(const float* a, const float* b, int64_t n, float scale,
                                   double* work, float* loss_out, float* da, int32_t accumulate,
                                   void* stream) {
  CLSKD_CHECK_ARG(a && b && work && loss_out, "mse_loss_grad: null pointer");
  CLSKD_CHECK_SHAPE(n > 0, "mse_loss_grad: n=%lld", (long long)n);
  CLSKD_CHECK_ARG(((uintptr_t)work & 7) == 0, "mse_loss_grad: work must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int nblk = mse_blocks(n);
  const float gscale = (float)((double)scale * 2.0 / (double)n);
  const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)da) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(mse_loss_grad_kernel<true>, dim3(nblk), dim3(256), 0, st, a, b, n, gscale, da,
                       accumulate, work);
  else
    hipLaunchKernelGGL(mse_loss_grad_kernel<false>, dim3(nblk), dim3(256), 0, st, a, b, n, gscale,
                       da, accumulate, work);
  hipLaunchKernelGGL(mse_loss_finalize_kernel, dim3(1), dim3(256), 0, st, work, nblk, n, scale,
                     loss_out, accumulate);
  CLSKD_LAUNCH_CHECK("mse_loss_grad");
  return CLSKD_OK;
}
