// ComplexBatchNorm (+ PReLU), forward and backward (tools_for_model.py:335-508, used at
// DCCRN.py:80,123 with use_cbn=True).  A BFTC row of C = 2*Cc floats holds the real parts of the
// Cc complex channels at [0, Cc) and the imaginary parts at [Cc, 2*Cc).  All passes are HBM-bound:
// a thread owns one quad of complex channels (one 16-B load of reals, one of imaginaries per
// row), statistics accumulate in fp64, reductions are two-level and fixed-order (reduce.h: no float
// atomics), per-channel algebra (V -> V^-1/2 -> Z, and its chain rule) runs in fp64 once per
// channel.  fp32 activations only.
//
// Per-channel tables (fp32, [k][Cc], 16-byte aligned):
//   coef  [6]: Zrr Zri Zir Zii Sr Si        y = Z x + S   (S = B - Z M)
//   stats [8]: Mr Mi Vrr Vri Vii Urr Uri Uii   (V with eps added, U = V^-1/2)
#include "common.h"
#include "reduce.h"

namespace clskd {

constexpr int CBN_NSTAT = 5;  // sum r, sum i, sum r^2, sum i^2, sum r*i
constexpr int CBN_NBWD = 7;   // sum gr, gi, gr*xhr, gr*xhi, gi*xhr, gi*xhi, PReLU term

// V (eps already added) -> U = V^-1/2 by the closed form of the 2x2 square root
// (tools_for_model.py:466-480): s = sqrt(det V), t = sqrt(tr V + 2s), U = adj(V + sI) / (s t).
struct CbnU {
  double s, t, rst, Urr, Uri, Uii;
};
__device__ __forceinline__ CbnU cbn_inv_sqrt(double Vrr, double Vri, double Vii) {
  CbnU u;
  u.s = sqrt(Vrr * Vii - Vri * Vri);
  u.t = sqrt(Vrr + Vii + 2.0 * u.s);
  u.rst = 1.0 / (u.s * u.t);
  u.Urr = (u.s + Vii) * u.rst;
  u.Uii = (u.s + Vrr) * u.rst;
  u.Uri = -Vri * u.rst;
  return u;
}

// The V -> Z step shared by the train finalize and the eval coefficients: coef (and stats when
// given) of complex channel c from its mean and its V without eps (tools_for_model.py:462-505).
__device__ __forceinline__ void cbn_channel_coeffs(int c, int Cc, double Mr, double Mi, double Vrr,
                                                   double Vri, double Vii, float eps,
                                                   const float* Wrr, const float* Wri,
                                                   const float* Wii, const float* Br,
                                                   const float* Bi, float* coef, float* stats) {
  Vrr += (double)eps;
  Vii += (double)eps;
  const CbnU u = cbn_inv_sqrt(Vrr, Vri, Vii);
  const double wrr = Wrr ? (double)Wrr[c] : 1.0, wri = Wri ? (double)Wri[c] : 0.0,
               wii = Wii ? (double)Wii[c] : 1.0;
  const double Zrr = wrr * u.Urr + wri * u.Uri, Zri = wrr * u.Uri + wri * u.Uii;
  const double Zir = wri * u.Urr + wii * u.Uri, Zii = wri * u.Uri + wii * u.Uii;
  coef[c] = (float)Zrr;
  coef[Cc + c] = (float)Zri;
  coef[2 * Cc + c] = (float)Zir;
  coef[3 * Cc + c] = (float)Zii;
  coef[4 * Cc + c] = (float)((Br ? (double)Br[c] : 0.0) - Zrr * Mr - Zri * Mi);
  coef[5 * Cc + c] = (float)((Bi ? (double)Bi[c] : 0.0) - Zir * Mr - Zii * Mi);
  if (stats) {
    stats[c] = (float)Mr;
    stats[Cc + c] = (float)Mi;
    stats[2 * Cc + c] = (float)Vrr;
    stats[3 * Cc + c] = (float)Vri;
    stats[4 * Cc + c] = (float)Vii;
    stats[5 * Cc + c] = (float)u.Urr;
    stats[6 * Cc + c] = (float)u.Uri;
    stats[7 * Cc + c] = (float)u.Uii;
  }
}

// y = Z x + S of one quad (the one expression every pass uses, so the backward sees the PReLU
// sign the forward saw)
struct CbnCoef {
  f32x4 zrr, zri, zir, zii, sr, si;
  __device__ __forceinline__ void load(const float* coef, int Cc, int c0) {
    zrr = load4<float>(coef + c0);
    zri = load4<float>(coef + Cc + c0);
    zir = load4<float>(coef + 2 * Cc + c0);
    zii = load4<float>(coef + 3 * Cc + c0);
    sr = load4<float>(coef + 4 * Cc + c0);
    si = load4<float>(coef + 5 * Cc + c0);
  }
  __device__ __forceinline__ void y(const f32x4& xr, const f32x4& xi, f32x4& yr, f32x4& yi) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      yr[j] = fmaf(zrr[j], xr[j], fmaf(zri[j], xi[j], sr[j]));
      yi[j] = fmaf(zir[j], xr[j], fmaf(zii[j], xi[j], si[j]));
    }
  }
};

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// block `blk` reduces rows [blk*rpb, (blk+1)*rpb) into partial[blk][Cc][5]
__global__ __launch_bounds__(256) void cbn_stats_partial_kernel(const float* __restrict__ x,
                                                                int64_t rows, int Cc, int64_t rpb,
                                                                double* __restrict__ partial) {
  const int CG = Cc >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int rl = tid / CG;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(rows, r0 + rpb);
  double acc[CBN_NSTAT][4];
#pragma unroll
  for (int k = 0; k < CBN_NSTAT; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[k][j] = 0.0;
  if (rl < RP) {
#pragma unroll 2
    for (int64_t r = r0 + rl; r < r1; r += RP) {
      const float* p = x + r * (2 * Cc) + cg * 4;
      const f32x4 vr = load4<float>(p), vi = load4<float>(p + Cc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double a = (double)vr[j], b = (double)vi[j];
        acc[0][j] += a;
        acc[1][j] += b;
        acc[2][j] += a * a;
        acc[3][j] += b * b;
        acc[4][j] += a * b;
      }
    }
  }
  row_lane_block_sum_2level<CBN_NSTAT>(acc, CG, RP,
                                       partial + (int64_t)blockIdx.x * Cc * CBN_NSTAT);
}

// one block per complex channel: moments in fp64, running buffers lerped n_updates times (V before
// eps, tools_for_model.py:433-457), then the shared V -> Z step
__global__ __launch_bounds__(256) void cbn_finalize_kernel(
    const double* __restrict__ partial, int nblk, int64_t rows, int Cc, const float* Wrr,
    const float* Wri, const float* Wii, const float* Br, const float* Bi, float eps, float* RMr,
    float* RMi, float* RVrr, float* RVri, float* RVii, float momentum, int n_updates, float* coef,
    float* stats) {
  const int c = blockIdx.x;
  double S[CBN_NSTAT];
  channel_partial_sum<CBN_NSTAT, 1>(partial, nblk, Cc, c, S);
  if (threadIdx.x != 0) return;
  const double n = (double)rows;
  const double Mr = S[0] / n, Mi = S[1] / n;
  double Vrr = S[2] / n - Mr * Mr, Vii = S[3] / n - Mi * Mi;
  const double Vri = S[4] / n - Mr * Mi;
  if (Vrr < 0) Vrr = 0;
  if (Vii < 0) Vii = 0;
  if (RMr && n_updates > 0) {
    float* run[5] = {RMr, RMi, RVrr, RVri, RVii};
    const float val[5] = {(float)Mr, (float)Mi, (float)Vrr, (float)Vri, (float)Vii};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float r = run[k][c];
      for (int u = 0; u < n_updates; ++u) r = r + momentum * (val[k] - r);  // Tensor.lerp_
      run[k][c] = r;
    }
  }
  cbn_channel_coeffs(c, Cc, Mr, Mi, Vrr, Vri, Vii, eps, Wrr, Wri, Wii, Br, Bi, coef, stats);
}

__global__ void cbn_eval_coeffs_kernel(const float* RMr, const float* RMi, const float* RVrr,
                                       const float* RVri, const float* RVii, const float* Wrr,
                                       const float* Wri, const float* Wii, const float* Br,
                                       const float* Bi, float eps, int Cc, float* coef,
                                       float* stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cc) return;
  cbn_channel_coeffs(c, Cc, (double)RMr[c], (double)RMi[c], (double)RVrr[c], (double)RVri[c],
                     (double)RVii[c], eps, Wrr, Wri, Wii, Br, Bi, coef, stats);
}

// y = Z x + S [then PReLU]; y may be x (each element is read and written by the same thread)
__global__ __launch_bounds__(256) void cbn_apply_kernel(const float* x, float* y, int64_t rows,
                                                        int Cc, int64_t rpb,
                                                        const float* __restrict__ coef,
                                                        const float* __restrict__ alpha) {
  const int CG = Cc >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int rl = tid / CG;
  if (rl >= RP) return;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(rows, r0 + rpb);
  const float al = alpha ? alpha[0] : 1.f;
  CbnCoef k;
  k.load(coef, Cc, cg * 4);
#pragma unroll 2
  for (int64_t r = r0 + rl; r < r1; r += RP) {
    const int64_t o = r * (2 * Cc) + cg * 4;
    const f32x4 xr = load4<float>(x + o), xi = load4<float>(x + o + Cc);
    f32x4 yr, yi;
    k.y(xr, xi, yr, yi);
    if (alpha) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        yr[j] = yr[j] > 0.f ? yr[j] : al * yr[j];
        yi[j] = yi[j] > 0.f ? yi[j] : al * yi[j];
      }
    }
    *reinterpret_cast<f32x4*>(y + o) = yr;
    *reinterpret_cast<f32x4*>(y + o + Cc) = yi;
  }
}

// ------------------------------------------------------------------------------------------
// backward.  With g = dy * prelu'(y) (torch's PReLU backward: slope alpha where y <= 0),
// xc = x - M, xh = U xc, y = W xh + B (W, U symmetric):
//   dB = sum g;  dWrr = sum gr*xhr, dWri = sum (gr*xhi + gi*xhr), dWii = sum gi*xhi
//   dalpha = sum over both parts and all channels of dy*y where y <= 0
//   dx = A g + K x + k with A = U W, K = [[2a, b], [b, 2c]] / n, k = -K M - A (sum g) / n,
//   (a, b, c) = dL/d(Vrr, Vri, Vii) by the chain rule through s, t, rst and U, fed with
//   dL/dU = W (sum g xh^T) U^-1 and U^-1 = V^1/2 = (V + sI) / t.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cbn_bwd_reduce_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int64_t rows, int Cc, int64_t rpb,
    const float* __restrict__ coef, const float* __restrict__ stats,
    const float* __restrict__ alpha, double* __restrict__ partial) {
  const int CG = Cc >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int rl = tid / CG;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(rows, r0 + rpb);
  const float al = alpha ? alpha[0] : 1.f;
  double acc[CBN_NBWD][4];
#pragma unroll
  for (int k = 0; k < CBN_NBWD; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[k][j] = 0.0;
  if (rl < RP) {
    CbnCoef k;
    k.load(coef, Cc, cg * 4);
    const f32x4 mr = load4<float>(stats + cg * 4), mi = load4<float>(stats + Cc + cg * 4);
    const f32x4 urr = load4<float>(stats + 5 * Cc + cg * 4);
    const f32x4 uri = load4<float>(stats + 6 * Cc + cg * 4);
    const f32x4 uii = load4<float>(stats + 7 * Cc + cg * 4);
    for (int64_t r = r0 + rl; r < r1; r += RP) {
      const int64_t o = r * (2 * Cc) + cg * 4;
      const f32x4 xr = load4<float>(x + o), xi = load4<float>(x + o + Cc);
      const f32x4 dr = load4<float>(dy + o), di = load4<float>(dy + o + Cc);
      f32x4 yr, yi;
      k.y(xr, xi, yr, yi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gr = dr[j], gi = di[j];
        if (alpha) {
          if (!(yr[j] > 0.f)) {
            acc[6][j] += (double)yr[j] * (double)dr[j];
            gr = al * dr[j];
          }
          if (!(yi[j] > 0.f)) {
            acc[6][j] += (double)yi[j] * (double)di[j];
            gi = al * di[j];
          }
        }
        const float cr = xr[j] - mr[j], ci = xi[j] - mi[j];
        const double hr = (double)fmaf(urr[j], cr, uri[j] * ci);
        const double hi = (double)fmaf(uri[j], cr, uii[j] * ci);
        acc[0][j] += (double)gr;
        acc[1][j] += (double)gi;
        acc[2][j] += (double)gr * hr;
        acc[3][j] += (double)gr * hi;
        acc[4][j] += (double)gi * hr;
        acc[5][j] += (double)gi * hi;
      }
    }
  }
  row_lane_block_sum_2level<CBN_NBWD>(acc, CG, RP,
                                      partial + (int64_t)blockIdx.x * Cc * CBN_NBWD);
}

// one block per complex channel; kc [9][Cc]: Arr Ari Air Aii Krr Kri Kii kr ki
__global__ __launch_bounds__(256) void cbn_bwd_finalize_kernel(
    const double* __restrict__ partial, int nblk, int64_t rows, int Cc, const float* stats,
    const float* Wrr, const float* Wri, const float* Wii, float* dWrr, float* dWri, float* dWii,
    float* dBr, float* dBi, float* kc, double* alpha_part, int accumulate) {
  const int c = blockIdx.x;
  double S[CBN_NBWD];
  channel_partial_sum<CBN_NBWD, 1>(partial, nblk, Cc, c, S);
  if (threadIdx.x != 0) return;
  const double n = (double)rows;
  const double Mr = stats[c], Mi = stats[Cc + c];
  const double p = stats[2 * Cc + c], q = stats[3 * Cc + c], r = stats[4 * Cc + c];
  const CbnU u = cbn_inv_sqrt(p, q, r);
  const double wrr = Wrr ? (double)Wrr[c] : 1.0, wri = Wri ? (double)Wri[c] : 0.0,
               wii = Wii ? (double)Wii[c] : 1.0;
  const double gBr = S[0], gBi = S[1];
  // G = W (sum g xh^T)
  const double Grr = wrr * S[2] + wri * S[4], Gri = wrr * S[3] + wri * S[5];
  const double Gir = wri * S[2] + wii * S[4], Gii = wri * S[3] + wii * S[5];
  // P = G U^-1, U^-1 = [[p + s, q], [q, r + s]] / t
  const double irr = (p + u.s) / u.t, iri = q / u.t, iii = (r + u.s) / u.t;
  const double Prr = Grr * irr + Gri * iri, Pri = Grr * iri + Gri * iii;
  const double Pir = Gir * irr + Gii * iri, Pii = Gir * iri + Gii * iii;
  const double gUrr = Prr, gUii = Pii, gUri = Pri + Pir;
  // chain rule through Urr = (s + r) rst, Uii = (s + p) rst, Uri = -q rst, rst = 1 / (s t),
  // t = sqrt(p + r + 2s), s = sqrt(p r - q^2)
  const double g_rst = gUrr * (u.s + r) + gUii * (u.s + p) - gUri * q;
  double g_s = (gUrr + gUii) * u.rst - g_rst * u.rst / u.s;
  const double g_t = -g_rst * u.rst / u.t;
  g_s += g_t / u.t;
  const double g_d = g_s / (2.0 * u.s);
  const double a = gUii * u.rst + g_t / (2.0 * u.t) + g_d * r;
  const double cc = gUrr * u.rst + g_t / (2.0 * u.t) + g_d * p;
  const double b = -gUri * u.rst - 2.0 * q * g_d;
  const double Krr = 2.0 * a / n, Kri = b / n, Kii = 2.0 * cc / n;
  const double Arr = u.Urr * wrr + u.Uri * wri, Ari = u.Urr * wri + u.Uri * wii;
  const double Air = u.Uri * wrr + u.Uii * wri, Aii = u.Uri * wri + u.Uii * wii;
  kc[c] = (float)Arr;
  kc[Cc + c] = (float)Ari;
  kc[2 * Cc + c] = (float)Air;
  kc[3 * Cc + c] = (float)Aii;
  kc[4 * Cc + c] = (float)Krr;
  kc[5 * Cc + c] = (float)Kri;
  kc[6 * Cc + c] = (float)Kii;
  kc[7 * Cc + c] = (float)(-(Krr * Mr + Kri * Mi) - (Arr * gBr + Ari * gBi) / n);
  kc[8 * Cc + c] = (float)(-(Kri * Mr + Kii * Mi) - (Air * gBr + Aii * gBi) / n);
  const float vWrr = (float)S[2], vWri = (float)(S[3] + S[4]), vWii = (float)S[5];
  if (dWrr) dWrr[c] = accumulate ? dWrr[c] + vWrr : vWrr;
  if (dWri) dWri[c] = accumulate ? dWri[c] + vWri : vWri;
  if (dWii) dWii[c] = accumulate ? dWii[c] + vWii : vWii;
  if (dBr) dBr[c] = accumulate ? dBr[c] + (float)gBr : (float)gBr;
  if (dBi) dBi[c] = accumulate ? dBi[c] + (float)gBi : (float)gBi;
  if (alpha_part) alpha_part[c] = S[6];
}

__global__ __launch_bounds__(256) void cbn_bwd_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int64_t rows, int Cc, int64_t rpb,
    const float* __restrict__ coef, const float* __restrict__ alpha, const float* __restrict__ kc,
    float* dx, int accumulate) {
  const int CG = Cc >> 2;
  const int RP = 256 / CG;
  const int tid = threadIdx.x;
  const int cg = tid % CG;
  const int rl = tid / CG;
  if (rl >= RP) return;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(rows, r0 + rpb);
  const float al = alpha ? alpha[0] : 1.f;
  CbnCoef k;
  k.load(coef, Cc, cg * 4);
  f32x4 A[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = load4<float>(kc + i * Cc + cg * 4);
#pragma unroll 2
  for (int64_t r = r0 + rl; r < r1; r += RP) {
    const int64_t o = r * (2 * Cc) + cg * 4;
    const f32x4 xr = load4<float>(x + o), xi = load4<float>(x + o + Cc);
    f32x4 gr = load4<float>(dy + o), gi = load4<float>(dy + o + Cc);
    if (alpha) {
      f32x4 yr, yi;
      k.y(xr, xi, yr, yi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!(yr[j] > 0.f)) gr[j] *= al;
        if (!(yi[j] > 0.f)) gi[j] *= al;
      }
    }
    f32x4 or_, oi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      or_[j] = fmaf(A[0][j], gr[j], fmaf(A[1][j], gi[j], fmaf(A[4][j], xr[j], fmaf(A[5][j], xi[j], A[7][j]))));
      oi[j] = fmaf(A[2][j], gr[j], fmaf(A[3][j], gi[j], fmaf(A[5][j], xr[j], fmaf(A[6][j], xi[j], A[8][j]))));
    }
    if (accumulate) {
      or_ += load4<float>(dx + o);
      oi += load4<float>(dx + o + Cc);
    }
    *reinterpret_cast<f32x4*>(dx + o) = or_;
    *reinterpret_cast<f32x4*>(dx + o + Cc) = oi;
  }
}

// blocks of a streaming pass: at least `per_thread` rows per thread, at most `cap` blocks
inline int32_t cbn_pass_blocks(int64_t rows, int32_t C, int64_t cap, int per_thread = 4) {
  const int CG = std::max(1, C / 8);
  const int RP = std::max(1, 256 / CG);
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(cap, cdiv(rows, (int64_t)RP * per_thread)));
}

inline bool cbn_shape_ok(int64_t rows, int32_t C) {
  return rows > 0 && C >= 8 && C % 8 == 0 && C <= 2048;
}

}  // namespace clskd

using namespace clskd;

extern "C" int32_t clskd_cbn_stats_blocks(int64_t rows, int32_t C) {
  return cbn_pass_blocks(rows, C, 2048, 8);  // a block's reduction tail amortised over more rows
}

extern "C" int clskd_cbn_stats_partial(const float* x, int64_t rows, int32_t C, double* partial,
                                       int32_t nblk, void* stream) {
  CLSKD_CHECK_ARG(x && partial, "cbn_stats: null pointer");
  CLSKD_CHECK_SHAPE(cbn_shape_ok(rows, C) && nblk >= 1, "cbn_stats: rows=%lld C=%d nblk=%d",
                    (long long)rows, C, nblk);
  CLSKD_CHECK_ARG(aligned16(x), "cbn_stats: x must be 16-byte aligned");
  hipLaunchKernelGGL(cbn_stats_partial_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), x, rows,
                     C / 2, cdiv(rows, nblk), partial);
  CLSKD_LAUNCH_CHECK("cbn_stats_partial");
  return CLSKD_OK;
}

extern "C" int clskd_cbn_finalize(const double* partial, int32_t nblk, int64_t rows, int32_t C,
                                  const float* Wrr, const float* Wri, const float* Wii,
                                  const float* Br, const float* Bi, float eps, float* RMr,
                                  float* RMi, float* RVrr, float* RVri, float* RVii,
                                  float momentum, int32_t n_updates, float* coef, float* stats,
                                  void* stream) {
  CLSKD_CHECK_ARG(partial && coef, "cbn_finalize: null pointer");
  CLSKD_CHECK_SHAPE(cbn_shape_ok(rows, C) && nblk >= 1, "cbn_finalize: rows=%lld C=%d nblk=%d",
                    (long long)rows, C, nblk);
  const bool run = RMr && RMi && RVrr && RVri && RVii;
  CLSKD_CHECK_ARG(run || !(RMr || RMi || RVrr || RVri || RVii),
                  "cbn_finalize: all five running buffers or none");
  hipLaunchKernelGGL(cbn_finalize_kernel, dim3(C / 2), dim3(256), 0, as_stream(stream), partial,
                     nblk, rows, C / 2, Wrr, Wri, Wii, Br, Bi, eps, RMr, RMi, RVrr, RVri, RVii,
                     momentum, run ? n_updates : 0, coef, stats);
  CLSKD_LAUNCH_CHECK("cbn_finalize");
  return CLSKD_OK;
}

extern "C" int clskd_cbn_eval_coeffs(const float* RMr, const float* RMi, const float* RVrr,
                                     const float* RVri, const float* RVii, const float* Wrr,
                                     const float* Wri, const float* Wii, const float* Br,
                                     const float* Bi, float eps, int32_t C, float* coef,
                                     float* stats, void* stream) {
  CLSKD_CHECK_ARG(RMr && RMi && RVrr && RVri && RVii && coef, "cbn_eval: null pointer");
  CLSKD_CHECK_SHAPE(cbn_shape_ok(1, C), "cbn_eval: C=%d", C);
  hipLaunchKernelGGL(cbn_eval_coeffs_kernel, dim3((unsigned)cdiv(C / 2, 256)), dim3(256), 0,
                     as_stream(stream), RMr, RMi, RVrr, RVri, RVii, Wrr, Wri, Wii, Br, Bi, eps,
                     C / 2, coef, stats);
  CLSKD_LAUNCH_CHECK("cbn_eval_coeffs");
  return CLSKD_OK;
}

extern "C" int clskd_cbn_apply(const float* x, float* y, int64_t rows, int32_t C,
                               const float* coef, const float* alpha, void* stream) {
  CLSKD_CHECK_ARG(x && y && coef, "cbn_apply: null pointer");
  CLSKD_CHECK_SHAPE(cbn_shape_ok(rows, C), "cbn_apply: rows=%lld C=%d", (long long)rows, C);
  CLSKD_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(coef), "cbn_apply: alignment");
  const int32_t nblk = cbn_pass_blocks(rows, C, 4096);
  hipLaunchKernelGGL(cbn_apply_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), x, y, rows,
                     C / 2, cdiv(rows, nblk), coef, alpha);
  CLSKD_LAUNCH_CHECK("cbn_apply");
  return CLSKD_OK;
}

extern "C" int32_t clskd_cbn_bwd_blocks(int64_t rows, int32_t C) {
  return cbn_pass_blocks(rows, C, 1024);
}

extern "C" int64_t clskd_cbn_bwd_workspace(int32_t nblk, int32_t C) {
  const int64_t Cc = C / 2;
  return (int64_t)nblk * Cc * CBN_NBWD + Cc + cdiv(9 * Cc, 2);  // doubles
}

extern "C" int clskd_cbn_bwd(const float* x, const float* dy, int64_t rows, int32_t C,
                             const float* coef, const float* stats, const float* Wrr,
                             const float* Wri, const float* Wii, const float* alpha, double* work,
                             int32_t nblk, float* dWrr, float* dWri, float* dWii, float* dBr,
                             float* dBi, float* dalpha, float* dx, int32_t accumulate_dx,
                             int32_t accumulate_params, void* stream) {
  CLSKD_CHECK_ARG(x && dy && coef && stats && work, "cbn_bwd: null pointer");
  CLSKD_CHECK_SHAPE(cbn_shape_ok(rows, C) && nblk >= 1, "cbn_bwd: rows=%lld C=%d nblk=%d",
                    (long long)rows, C, nblk);
  CLSKD_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(coef) && aligned16(stats) &&
                      aligned16(work) && (!dx || aligned16(dx)),
                  "cbn_bwd: x, dy, dx, coef, stats and work must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int Cc = C / 2;
  // work layout: partial[nblk][Cc][7] | alpha_part[Cc] | kc[9][Cc] (floats)
  double* partial = work;
  double* apart = work + (int64_t)nblk * Cc * CBN_NBWD;
  float* kc = reinterpret_cast<float*>(apart + Cc);
  const int64_t rpb = cdiv(rows, nblk);
  hipLaunchKernelGGL(cbn_bwd_reduce_kernel, dim3(nblk), dim3(256), 0, st, x, dy, rows, Cc, rpb,
                     coef, stats, alpha, partial);
  hipLaunchKernelGGL(cbn_bwd_finalize_kernel, dim3(Cc), dim3(256), 0, st, partial, nblk, rows, Cc,
                     stats, Wrr, Wri, Wii, dWrr, dWri, dWii, dBr, dBi, kc,
                     alpha ? apart : nullptr, accumulate_params);
  if (alpha && dalpha)
    bn_bwd_alpha(apart, Cc, 1, dalpha, accumulate_params, st);
  if (dx) {
    const int32_t nb = cbn_pass_blocks(rows, C, 4096);
    hipLaunchKernelGGL(cbn_bwd_apply_kernel, dim3(nb), dim3(256), 0, st, x, dy, rows, Cc,
                       cdiv(rows, nb), coef, alpha, kc, dx, accumulate_dx);
  }
  CLSKD_LAUNCH_CHECK("cbn_bwd");
  return CLSKD_OK;
}
