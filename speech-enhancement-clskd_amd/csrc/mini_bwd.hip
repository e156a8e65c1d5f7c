// Backward kernels of the asteroid DCCRNet_mini training step that have no counterpart in the
// local-DCCRN backward (norm_bwd.hip): the bounded complex mask times the spectrum, the OnReIm
// BatchNorm + PReLU pair (one slope per part) and the output-level MSE distillation loss.
// HBM-bound passes; every reduction is fp64 partials combined in a fixed order (no float atomics,
// no agent-scope fences), so gradients and losses are bitwise repeatable.
#include <algorithm>

#include "common.h"

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
// OnReIm(BatchNorm2d, train) + OnReIm(PReLU) backward over BFTC x [rows][C]: clskd_bn_bwd
// (norm_bwd.hip: the formulas and the partial-then-finalize scheme are its own) with the slope
// alpha[0] on channels [0, C/2) and alpha[1] on [C/2, C), and one slope gradient per half.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_reim_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int64_t rows, int C, int64_t rpb,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ mean, const float* __restrict__ var, float eps,
    const float* __restrict__ alpha, double* __restrict__ partial) {
  const int CG = C >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int rl = tid / CG;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(rows, r0 + rpb);
  f32x4 sc, sh, mu, rs, al;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = cg * 4 + j;
    sc[j] = scale[c];
    sh[j] = shift[c];
    mu[j] = mean[c];
    rs[j] = (float)(1.0 / sqrt((double)var[c] + (double)eps));
    al[j] = alpha[2 * c >= C ? 1 : 0];
  }
  double sb[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sa[4] = {0, 0, 0, 0};
  if (rl < RP) {
    for (int64_t r = r0 + rl; r < r1; r += RP) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * C + cg * 4);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(dy + r * C + cg * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float yb = fmaf(xv[j], sc[j], sh[j]);
        float dz = gv[j];
        if (!(yb > 0.f)) {
          sa[j] += (double)yb * (double)gv[j];
          dz = al[j] * gv[j];
        }
        const float xh = (xv[j] - mu[j]) * rs[j];
        sb[j] += (double)dz;
        sg[j] += (double)dz * (double)xh;
      }
    }
  }
  __shared__ double red[256][13];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[tid][j] = sb[j];
    red[tid][4 + j] = sg[j];
    red[tid][8 + j] = sa[j];
  }
  __syncthreads();
  if (tid < CG) {
    double Bv[4] = {0, 0, 0, 0}, G[4] = {0, 0, 0, 0}, A[4] = {0, 0, 0, 0};
    for (int l = 0; l < RP; ++l) {
      const int t = l * CG + tid;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        Bv[j] += red[t][j];
        G[j] += red[t][4 + j];
        A[j] += red[t][8 + j];
      }
    }
    double* p = partial + ((int64_t)blockIdx.x * C + tid * 4) * 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p[3 * j] = Bv[j];
      p[3 * j + 1] = G[j];
      p[3 * j + 2] = A[j];
    }
  }
}

// one block per channel: dgamma / dbeta (accumulate optional), k[3][C], alpha_part[C]
__global__ __launch_bounds__(256) void bn_bwd_reim_finalize_kernel(
    const double* __restrict__ partial, int nblk, int64_t rows, int C, const float* gamma,
    const float* mean, const float* var, float eps, float* dgamma, float* dbeta, float* k,
    double* alpha_part, int accumulate) {
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  double sb = 0, sg = 0, sa = 0;
  for (int b = tid; b < nblk; b += 256) {
    const double* p = partial + ((int64_t)b * C + c) * 3;
    sb += p[0];
    sg += p[1];
    sa += p[2];
  }
  __shared__ double r0[256], r1[256], r2[256];
  r0[tid] = sb;
  r1[tid] = sg;
  r2[tid] = sa;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      r0[tid] += r0[tid + o];
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double SB = r0[0], SG = r1[0];
    const double n = (double)rows;
    const double rs = 1.0 / sqrt((double)var[c] + (double)eps);
    const double g = gamma ? (double)gamma[c] : 1.0;
    k[c] = (float)(g * rs);
    k[C + c] = (float)(-g * rs * rs * SG / n);
    k[2 * C + c] = (float)(-g * rs * SB / n + g * rs * rs * (double)mean[c] * SG / n);
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)SG : (float)SG;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)SB : (float)SB;
    alpha_part[c] = r2[0];
  }
}

// dalpha[h] (+)= sum of alpha_part over the channels of half h, ascending (fixed order)
__global__ void bn_bwd_reim_alpha_kernel(const double* alpha_part, int C, float* dalpha,
                                         int accumulate) {
  const int h = threadIdx.x;
  if (blockIdx.x == 0 && h < 2) {
    double s = 0;
    for (int c = h * (C / 2); c < (h + 1) * (C / 2); ++c) s += alpha_part[c];
    dalpha[h] = accumulate ? dalpha[h] + (float)s : (float)s;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_reim_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int64_t rows, int C,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ alpha, const float* __restrict__ k, float* __restrict__ dx,
    int accumulate) {
  const int64_t nq = rows * C / 4;
  const float a0 = alpha[0], a1 = alpha[1];
  // channel of the thread's first quad, advanced by the grid stride (mod C) as in
  // bn_bwd_apply_kernel; the per-channel vectors are 16-B loads (C % 4 == 0, 16-B aligned: host)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cstep = (int)((stride * 4) % C);
  int c0 = (int)((q0 * 4) % C);
  for (int64_t q = q0; q < nq; q += stride) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + q * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(dy + q * 4);
    const f32x4 k0 = *reinterpret_cast<const f32x4*>(k + c0);
    const f32x4 k1 = *reinterpret_cast<const f32x4*>(k + C + c0);
    const f32x4 k2 = *reinterpret_cast<const f32x4*>(k + 2 * C + c0);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c0);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c0);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float dz = gv[j];
      if (!(fmaf(xv[j], sc[j], sh[j]) > 0.f)) dz *= 2 * (c0 + j) >= C ? a1 : a0;
      o[j] = fmaf(k0[j], dz, fmaf(k1[j], xv[j], k2[j]));
    }
    c0 += cstep;
    if (c0 >= C) c0 -= C;
    if (accumulate) o += *reinterpret_cast<const f32x4*>(dx + q * 4);
    *reinterpret_cast<f32x4*>(dx + q * 4) = o;
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
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// loss_out (+)= scale * (sum of the block partials, fixed order) / n
__global__ __launch_bounds__(256) void mse_loss_finalize_kernel(const double* __restrict__ partial,
                                                               int nblk, int64_t n, float scale,
                                                               float* loss_out, int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = (float)((double)scale * red[0] / (double)n);
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

extern "C" int clskd_bn_bwd_reim(const float* x, const float* dy, int64_t rows, int32_t C,
                                 const float* scale, const float* shift, const float* mean,
                                 const float* var, float eps, const float* gamma,
                                 const float* alpha_re_im, double* work, int32_t nblk,
                                 float* dgamma, float* dbeta, float* dalpha_re_im, float* dx,
                                 int32_t accumulate_dx, int32_t accumulate_params, void* stream) {
  CLSKD_CHECK_ARG(x && dy && scale && shift && mean && var && alpha_re_im && work && dx,
                  "bn_bwd_reim: null pointer");
  CLSKD_CHECK_SHAPE(rows > 0 && C >= 4 && C % 4 == 0 && C <= 1024 && nblk >= 1,
                    "bn_bwd_reim: rows=%lld C=%d nblk=%d (C: a multiple of 4, two equal halves)",
                    (long long)rows, C, nblk);
  CLSKD_CHECK_ARG(((uintptr_t)work & 15) == 0 && ((uintptr_t)scale & 15) == 0 &&
                      ((uintptr_t)shift & 15) == 0 && ((uintptr_t)x & 15) == 0 &&
                      ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dx & 15) == 0,
                  "bn_bwd_reim: x, dy, dx, scale, shift and work must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  // work layout of clskd_bn_bwd: partial[nblk][C][3] | k[3C] (as floats) | alpha_part[C]
  double* partial = work;
  float* k = reinterpret_cast<float*>(work + (int64_t)nblk * C * 3);
  double* apart = work + (int64_t)nblk * C * 3 + cdiv(3 * C, 2);
  const int64_t rpb = cdiv(rows, nblk);
  hipLaunchKernelGGL(bn_bwd_reim_reduce_kernel, dim3(nblk), dim3(256), 0, st, x, dy, rows, C, rpb,
                     scale, shift, mean, var, eps, alpha_re_im, partial);
  hipLaunchKernelGGL(bn_bwd_reim_finalize_kernel, dim3(C), dim3(256), 0, st, partial, nblk, rows, C,
                     gamma, mean, var, eps, dgamma, dbeta, k, apart, accumulate_params);
  if (dalpha_re_im)
    hipLaunchKernelGGL(bn_bwd_reim_alpha_kernel, dim3(1), dim3(64), 0, st, apart, C, dalpha_re_im,
                       accumulate_params);
  const int64_t nq = rows * C / 4;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(nq, 256), 8192));
  hipLaunchKernelGGL(bn_bwd_reim_apply_kernel, dim3(grid), dim3(256), 0, st, x, dy, rows, C, scale,
                     shift, alpha_re_im, k, dx, accumulate_dx);
  CLSKD_LAUNCH_CHECK("bn_bwd_reim");
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
