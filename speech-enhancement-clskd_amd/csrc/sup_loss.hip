// Supervised losses of DCCRN.loss (DCCRN.py:259-411) and their gradients: the waveform terms
// MSE / SDR / SI-SNR / SI-SDR (tools_for_loss.py:22-97) from one pass of per-row sums, and the
// mel log-spectral distance "LMS" (tools_for_loss.py:195-252) with its backward.
//
// Waveform terms.  With A = sum s^2, Y = sum y^2, C = sum s y and D = sum (s - y)^2 per row, every
// term is a function of (A, Y, C, D) and of batch means of such functions, so
//   dL/ds_b = p_b s_b + q_b y_b = p_b (s_b - y_b) + (p_b + q_b) y_b
// with per-row scalars: one sums pass (fp64 block partials), one finalize launch (values + the
// [B][2] coefficient table, already weighted and multiplied by upstream), one axpby pass.
// D is accumulated from the differences themselves: A - 2C + Y cancels when s ~ y.  The residual
// energies sum (s - a y)^2 are rebuilt around D, sum (s - a y)^2 = D + 2u(C - Y) + u^2 Y with
// u = 1 - a, which keeps their digits at high SNR for the same reason.
//
// LMS.  perceptual_transform views the contiguous [257][T] magnitudes of one clip as (-1, 257):
// row r is the flat run [257 r, 257 r + 257) of the frequency-major array, flat n = f T + t, and
// filter position j is the offset inside that run (not a frequency bin).  The spectra live
// frame-major ([B][T][ld], re at f, im at 257 + f), so a run is a strided gather; a workgroup
// takes MEL_ROWS consecutive rows = one flat range, walks the (t, f) rectangle that covers it with
// f fastest (contiguous HBM runs of the rectangle's width) and keeps the magnitudes in LDS by flat
// offset.  No float atomics, no fences: fp64 block partials, a finalize launch.
#include <algorithm>

#include "common.h"
#include "reduce.h"

namespace clskd {

constexpr int WL_CHUNK_MAX = 64;   // blocks per row of the sums pass
constexpr int WL_QUADS = 4;        // 16-byte pieces per thread per sweep
constexpr double LOG10_K = 4.342944819032518;  // 10 / ln 10

struct WaveW {
  float w[5];
};

__device__ __forceinline__ void wl_acc(float s, float y, double& a, double& b, double& c,
                                       double& d) {
  const double sd = (double)s, yd = (double)y, e = sd - yd;
  a += sd * sd;
  b += yd * yd;
  c += sd * yd;
  d += e * e;
}

// Rows whose s and y start at the same offset from a 16-byte boundary run on 16-byte loads with a
// scalar head (< 4 elements) and tail; other rows scalar.  Uniform per block.
__device__ __forceinline__ int row_head(const float* p, int L) {
  const int h = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);
  return h < L ? h : L;
}

// grid (nchunk, B): block (c, b) sums the pieces q = c*256 + tid, += nchunk*256 of row b.
__global__ __launch_bounds__(256) void wave_sums_kernel(const float* __restrict__ s, int64_t lds,
                                                        const float* __restrict__ y, int64_t ldy,
                                                        int L, double* __restrict__ partial) {
  const int b = blockIdx.y, c = blockIdx.x, nchunk = gridDim.x;
  const float* sr = s + (int64_t)b * lds;
  const float* yr = y + (int64_t)b * ldy;
  double A = 0, Y = 0, Cc = 0, D = 0;
  const bool vec = ((((uintptr_t)sr) ^ ((uintptr_t)yr)) & 15) == 0;
  if (vec) {
    const int h = row_head(sr, L);
    const int nq = (L - h) >> 2;
    const int t0 = h + 4 * nq;
    if (c == 0) {
      if ((int)threadIdx.x < h) wl_acc(sr[threadIdx.x], yr[threadIdx.x], A, Y, Cc, D);
      if ((int)threadIdx.x < L - t0) wl_acc(sr[t0 + threadIdx.x], yr[t0 + threadIdx.x], A, Y, Cc, D);
    }
    for (int q = c * 256 + threadIdx.x; q < nq; q += nchunk * 256) {
      const f32x4 sv = *reinterpret_cast<const f32x4*>(sr + h + 4 * (int64_t)q);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(yr + h + 4 * (int64_t)q);
#pragma unroll
      for (int i = 0; i < 4; ++i) wl_acc(sv[i], yv[i], A, Y, Cc, D);
    }
  } else {
    for (int i = c * 256 + threadIdx.x; i < L; i += nchunk * 256) wl_acc(sr[i], yr[i], A, Y, Cc, D);
  }
  A = wave_sum_d(A);
  Y = wave_sum_d(Y);
  Cc = wave_sum_d(Cc);
  D = wave_sum_d(D);
  __shared__ double red[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = A;
    red[w][1] = Y;
    red[w][2] = Cc;
    red[w][3] = D;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partial[((int64_t)b * nchunk + c) * 4 + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// residual energy sum (e - a r)^2 around D: Er = sum r^2, X = sum r e, D = sum (e - r)^2
__device__ __forceinline__ double resid(double D, double X, double Er, double a) {
  const double u = 1.0 - a;
  return D + 2.0 * u * (X - Er) + u * u * Er;
}

// One block.  rows[B][4] = (A, Y, C, D) per row (the partials' fixed-order sums); then the five
// values, out[0] = sum w_k l_k, and the coefficient table.
__global__ __launch_bounds__(256) void wave_finalize_kernel(const double* __restrict__ partial,
                                                            int nchunk, int B, int L, WaveW ww,
                                                            float upstream,
                                                            double* __restrict__ rows,
                                                            float* __restrict__ out,
                                                            float* __restrict__ coef) {
  const double eps = 1e-8;
  double sD = 0, sSdr = 0, sSnr = 0, sR3 = 0, sR4 = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    double v[4] = {0, 0, 0, 0};
    for (int c = 0; c < nchunk; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += partial[((int64_t)b * nchunk + c) * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rows[(int64_t)b * 4 + k] = v[k];
    const double A = v[0], Y = v[1], C = v[2], D = v[3];
    sD += D;
    sSdr += LOG10_K * log(Y * Y / (D * D + eps));
    {  // si_snr(s, y)
      const double a = C / (Y + eps);
      sSnr += LOG10_K * log(a * a * Y / (resid(D, C, Y, a) + eps) + eps);
    }
    {  // si_sdr(reference = y, estimation = s): the ratio, averaged before the log
      const double a = C / Y + eps;
      sR3 += a * a * Y / resid(D, C, Y, a) + eps;
    }
    {  // si_sdr(reference = s, estimation = y)
      const double a = C / A + eps;
      sR4 += a * a * A / resid(D, C, A, a) + eps;
    }
  }
  double tot[5] = {sD, sSdr, sSnr, sR3, sR4};
  block_tree_sum<5>(tot);
  const double tD = tot[0], tSdr = tot[1], tSnr = tot[2];
  const double R3 = tot[3] / (double)B, R4 = tot[4] / (double)B;
  const double invB = 1.0 / (double)B, invN = 1.0 / ((double)B * (double)L);
  if (threadIdx.x == 0) {
    const double l[5] = {tD * invN, -tSdr * invB, -tSnr * invB, -LOG10_K * log(R3 + eps),
                         -LOG10_K * log(R4 + eps)};
    double tot = 0;
    for (int k = 0; k < 5; ++k) {
      out[1 + k] = (float)l[k];
      if (ww.w[k] != 0.f) tot += (double)ww.w[k] * l[k];
    }
    out[0] = (float)tot;
  }
  if (!coef) return;
  const double K3 = LOG10_K / ((R3 + eps) * (double)B), K4 = LOG10_K / ((R4 + eps) * (double)B);
  for (int b = threadIdx.x; b < B; b += 256) {
    const double A = rows[(int64_t)b * 4], Y = rows[(int64_t)b * 4 + 1];
    const double C = rows[(int64_t)b * 4 + 2], D = rows[(int64_t)b * 4 + 3];
    double p = 0, q = 0;
    if (ww.w[0] != 0.f) {
      p += (double)ww.w[0] * 2.0 * invN;
      q -= (double)ww.w[0] * 2.0 * invN;
    }
    if (ww.w[1] != 0.f) {
      const double k1 = (double)ww.w[1] * 4.0 * LOG10_K * D / (D * D + eps) * invB;
      p += k1;
      q -= k1;
    }
    if (ww.w[2] != 0.f) {
      const double Ye = Y + eps, a = C / Ye, Tn = a * a * Y;
      const double Ne = resid(D, C, Y, a) + eps, r = Tn / Ne + eps;
      const double K2 = (double)ww.w[2] * LOG10_K * invB / r;
      p += K2 * 2.0 * Tn / (Ne * Ne);
      q -= K2 * (2.0 * a * Y / (Ye * Ne) + Tn / (Ne * Ne) * (2.0 * a + 2.0 * (C - a * Y) / Ye));
    }
    if (ww.w[3] != 0.f) {
      const double a = C / Y + eps, P = a * a * Y, Nz = resid(D, C, Y, a);
      p += (double)ww.w[3] * K3 * 2.0 * P / (Nz * Nz);
      q -= (double)ww.w[3] * K3 * (2.0 * a / Nz + P / (Nz * Nz) * (2.0 * a - 2.0 * eps));
    }
    if (ww.w[4] != 0.f) {
      const double c1 = C / A, a = c1 + eps, P = a * a * A, Nz = resid(D, C, A, a);
      const double g = C - a * A;
      const double ps = (-4.0 * a * c1 + 2.0 * a * a) / Nz - P / (Nz * Nz) * (2.0 * a * a + 4.0 * g * c1 / A);
      const double qs = 2.0 * a / Nz + P / (Nz * Nz) * (2.0 * a + 2.0 * g / A);
      p -= (double)ww.w[4] * K4 * ps;
      q -= (double)ww.w[4] * K4 * qs;
    }
    // stored as (p, r = p + q): the gradient pass forms p (s - y) + r y, which does not cancel
    // when s ~ y (MSE and SDR have r = 0 exactly)
    coef[2 * b] = (float)((double)upstream * p);
    coef[2 * b + 1] = (float)((double)upstream * (p + q));
  }
}

// d[b] (+)= p_b s_b + q_b y_b, evaluated as p_b (s_b - y_b) + r_b y_b from the table's (p_b, r_b);
// grid (nchunk, B).  16-byte accesses when the three rows share their offset from a 16-byte
// boundary.
__global__ __launch_bounds__(256) void wave_grad_kernel(const float* __restrict__ s, int64_t lds,
                                                        const float* __restrict__ y, int64_t ldy,
                                                        int L, const float* __restrict__ coef,
                                                        float* __restrict__ d, int64_t ldd,
                                                        int accumulate) {
  const int b = blockIdx.y, c = blockIdx.x, nchunk = gridDim.x;
  const float* sr = s + (int64_t)b * lds;
  const float* yr = y + (int64_t)b * ldy;
  float* dr = d + (int64_t)b * ldd;
  const float p = coef[2 * b], r = coef[2 * b + 1];
  const bool vec = (((((uintptr_t)sr) ^ ((uintptr_t)yr)) | (((uintptr_t)sr) ^ ((uintptr_t)dr))) & 15) == 0;
  if (vec) {
    const int h = row_head(sr, L);
    const int nq = (L - h) >> 2;
    const int t0 = h + 4 * nq;
    if (c == 0) {
      const int t = threadIdx.x;
      if (t < h) {
        const float v = fmaf(p, sr[t] - yr[t], r * yr[t]);
        dr[t] = accumulate ? dr[t] + v : v;
      }
      if (t < L - t0) {
        const float v = fmaf(p, sr[t0 + t] - yr[t0 + t], r * yr[t0 + t]);
        dr[t0 + t] = accumulate ? dr[t0 + t] + v : v;
      }
    }
    for (int k = c * 256 + threadIdx.x; k < nq; k += nchunk * 256) {
      const int64_t o = h + 4 * (int64_t)k;
      const f32x4 sv = *reinterpret_cast<const f32x4*>(sr + o);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(yr + o);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaf(p, sv[i] - yv[i], r * yv[i]);
      if (accumulate) v += *reinterpret_cast<const f32x4*>(dr + o);
      *reinterpret_cast<f32x4*>(dr + o) = v;
    }
  } else {
    for (int i = c * 256 + threadIdx.x; i < L; i += nchunk * 256) {
      const float v = fmaf(p, sr[i] - yr[i], r * yr[i]);
      dr[i] = accumulate ? dr[i] + v : v;
    }
  }
}

inline int wave_chunks(int L) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(WL_CHUNK_MAX, cdiv(L, 256 * 4 * WL_QUADS)));
}

// ------------------------------------------------------------------------------------------
// LMS
// ------------------------------------------------------------------------------------------
constexpr int MEL_NB = 257;                    // positions of a row
constexpr int MEL_NF = CLSKD_MEL_FILTERS;      // 16 + 32 + 64 filters
constexpr int MEL_ROWS = 32;                   // rows of a workgroup
constexpr int MEL_HALF = MEL_ROWS / 2;
constexpr float MEL_EPS = 1e-7f;
// table words (include/clskd.h): dense filters, supports, per-position pairs
constexpr int MT_W = 0;
constexpr int MT_SUPP = MT_W + MEL_NF * MEL_NB;
constexpr int MT_PK = MT_SUPP + MEL_NF * 2;
constexpr int MT_PW = MT_PK + MEL_NB * 6;
constexpr int MT_WORDS = MT_PW + MEL_NB * 6;
static_assert(MT_WORDS == CLSKD_MEL_TABLE_WORDS, "mel table layout");

__device__ __forceinline__ int mel_scale_of(int k) { return k < 16 ? 0 : (k < 48 ? 1 : 2); }
__device__ __forceinline__ int mel_scale_n(int sc) { return 16 << sc; }

struct MelRange {
  int n0, n1;     // flat range [n0, n1) of the clip's [257][T] magnitudes
  int f_lo, fw;   // covering rectangle: frequencies [f_lo, f_lo + fw) x every frame
  int nrows;
};

__device__ __forceinline__ MelRange mel_range(int T) {
  MelRange g;
  const int r0 = blockIdx.x * MEL_ROWS;
  g.nrows = min(MEL_ROWS, T - r0);
  g.n0 = r0 * MEL_NB;
  g.n1 = g.n0 + g.nrows * MEL_NB;
  g.f_lo = g.n0 / T;
  g.fw = (g.n1 - 1) / T - g.f_lo + 1;
  return g;
}

// magnitudes sqrt(re^2 + im^2 + 1e-7) / 512 of the block's flat range into m[n - n0].  MEL_U
// elements per thread per sweep, every load issued before the first use: with one workgroup per
// CU a load per iteration would expose a full memory latency each time.
constexpr int MEL_U = 8;

__device__ __forceinline__ void mel_stage(const float* __restrict__ x, int ld, int T,
                                          const MelRange& g, float* __restrict__ m) {
  const int total = T * g.fw;
  for (int base = threadIdx.x; base < total; base += 256 * MEL_U) {
    float re[MEL_U], im[MEL_U];
    int loc[MEL_U];
#pragma unroll
    for (int u = 0; u < MEL_U; ++u) {
      const int idx = base + u * 256;
      loc[u] = -1;
      re[u] = im[u] = 0.f;
      if (idx < total) {
        const int t = idx / g.fw, f = g.f_lo + (idx - t * g.fw);
        const int n = f * T + t;
        if (n >= g.n0 && n < g.n1) {
          loc[u] = n - g.n0;
          re[u] = x[(int64_t)t * ld + f];
          im[u] = x[(int64_t)t * ld + MEL_NB + f];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < MEL_U; ++u)
      if (loc[u] >= 0) m[loc[u]] = sqrtf(re[u] * re[u] + im[u] * im[u] + MEL_EPS) * (1.0f / 512.0f);
  }
}

// Thread (k, half) for k < 112: filter k over its support for 16 rows of both spectra (fp64
// accumulators), then delta[r][k] = log(pe + 1e-7) - log(pc + 1e-7) and inv[r][k] = 1 / (pe + 1e-7).
__device__ __forceinline__ void mel_project(const uint32_t* __restrict__ tab,
                                            const float* __restrict__ mc,
                                            const float* __restrict__ me, int nrows,
                                            double* __restrict__ delta, float* __restrict__ inv) {
  const int k = threadIdx.x >> 1, half = threadIdx.x & 1;
  if (k >= MEL_NF) return;
  const float* W = reinterpret_cast<const float*>(tab + MT_W) + k * MEL_NB;
  const int js = max(0, (int)tab[MT_SUPP + 2 * k]);
  const int je = min(MEL_NB, (int)tab[MT_SUPP + 2 * k + 1]);
  double ac[MEL_HALF], ae[MEL_HALF];
#pragma unroll
  for (int r = 0; r < MEL_HALF; ++r) ac[r] = ae[r] = 0.0;
  const float* pc = mc + half * MEL_HALF * MEL_NB;
  const float* pe = me + half * MEL_HALF * MEL_NB;
  for (int j = js; j < je; ++j) {
    const double w = (double)W[j];
#pragma unroll
    for (int r = 0; r < MEL_HALF; ++r) {
      ac[r] += w * (double)pc[r * MEL_NB + j];
      ae[r] += w * (double)pe[r * MEL_NB + j];
    }
  }
#pragma unroll
  for (int r = 0; r < MEL_HALF; ++r) {
    const int row = half * MEL_HALF + r;
    if (row < nrows) {
      const double e = ae[r] + (double)MEL_EPS, c = ac[r] + (double)MEL_EPS;
      delta[row * MEL_NF + k] = log(e) - log(c);
      if (inv) inv[row * MEL_NF + k] = (float)(1.0 / e);
    }
  }
}

// row value sqrt(mean_k delta^2 + 1e-7) of (row, scale), filters summed in index order
__device__ __forceinline__ double mel_rowval(const double* __restrict__ delta, int row, int sc) {
  const int k0 = sc == 0 ? 0 : (sc == 1 ? 16 : 48), n = mel_scale_n(sc);
  double v = 0;
  for (int k = 0; k < n; ++k) {
    const double d = delta[row * MEL_NF + k0 + k];
    v += d * d;
  }
  return sqrt(v / (double)n + (double)MEL_EPS);
}

constexpr size_t MEL_LDS_FWD = 2 * MEL_ROWS * MEL_NB * sizeof(float) + MEL_ROWS * MEL_NF * sizeof(double);
constexpr size_t MEL_LDS_BWD = MEL_LDS_FWD + MEL_ROWS * MEL_NF * sizeof(float);

// grid (ceil(T / MEL_ROWS), B): partial[b * gridDim.x + blockIdx.x] = sum of the block's
// (row, scale) values.  The zero-filled pad rows of a ragged block are never read back.
__global__ __launch_bounds__(256) void mel_fwd_kernel(const float* __restrict__ clean, int ldc,
                                                      const float* __restrict__ est, int lde, int T,
                                                      const uint32_t* __restrict__ tab,
                                                      double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* mc = reinterpret_cast<float*>(smem);
  float* me = mc + MEL_ROWS * MEL_NB;
  double* delta = reinterpret_cast<double*>(me + MEL_ROWS * MEL_NB);
  const MelRange g = mel_range(T);
  const int b = blockIdx.y;
  for (int i = g.nrows * MEL_NB + threadIdx.x; i < MEL_ROWS * MEL_NB; i += 256) mc[i] = me[i] = 0.f;
  mel_stage(clean + (int64_t)b * T * ldc, ldc, T, g, mc);
  mel_stage(est + (int64_t)b * T * lde, lde, T, g, me);
  __syncthreads();
  mel_project(tab, mc, me, g.nrows, delta, nullptr);
  __syncthreads();
  double v = 0;
  if ((int)threadIdx.x < 3 * g.nrows) v = mel_rowval(delta, threadIdx.x / 3, threadIdx.x % 3);
  const double tot = block_tree_sum(v);
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = tot;
}

// out2[0] (+)= scale * mean, out2[1] = mean, over count = 3 B T (row, scale) values
__global__ __launch_bounds__(256) void mel_finalize_kernel(const double* __restrict__ partial,
                                                           int64_t n, double count, float scale,
                                                           int accumulate, float* out2) {
  double s = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += partial[i];
  const double tot = block_tree_sum(s);
  if (threadIdx.x == 0) {
    const float mean = (float)(tot / count);
    const float v = (float)((double)scale * (tot / count));
    out2[0] = accumulate ? out2[0] + v : v;
    out2[1] = mean;
  }
}

// d est (+)= gscale * d(sum of row values) / d est, gscale = upstream / (3 B T): the projections
// recomputed, a[r][k] = delta / (S rowval (pe + 1e-7)) per filter, then per position the (at most
// six) filters that cover it, and d m / d re = re / (512^2 m).
__global__ __launch_bounds__(256) void mel_bwd_kernel(const float* __restrict__ clean, int ldc,
                                                      const float* __restrict__ est, int lde, int T,
                                                      const uint32_t* __restrict__ tab, float gscale,
                                                      float* __restrict__ dest, int ldd,
                                                      int accumulate) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* mc = reinterpret_cast<float*>(smem);
  float* me = mc + MEL_ROWS * MEL_NB;
  double* delta = reinterpret_cast<double*>(me + MEL_ROWS * MEL_NB);
  float* av = reinterpret_cast<float*>(delta + MEL_ROWS * MEL_NF);
  __shared__ double rv[MEL_ROWS * 3];
  const MelRange g = mel_range(T);
  const int b = blockIdx.y;
  const float* eb = est + (int64_t)b * T * lde;
  for (int i = g.nrows * MEL_NB + threadIdx.x; i < MEL_ROWS * MEL_NB; i += 256) mc[i] = me[i] = 0.f;
  mel_stage(clean + (int64_t)b * T * ldc, ldc, T, g, mc);
  mel_stage(eb, lde, T, g, me);
  __syncthreads();
  mel_project(tab, mc, me, g.nrows, delta, av);
  __syncthreads();
  if ((int)threadIdx.x < 3 * g.nrows) rv[threadIdx.x] = mel_rowval(delta, threadIdx.x / 3, threadIdx.x % 3);
  __syncthreads();
  for (int i = threadIdx.x; i < g.nrows * MEL_NF; i += 256) {
    const int row = i / MEL_NF, k = i - row * MEL_NF, sc = mel_scale_of(k);
    av[i] = (float)((double)gscale * delta[i] * (double)av[i] /
                    ((double)mel_scale_n(sc) * rv[row * 3 + sc]));
  }
  __syncthreads();
  const int32_t* pk = reinterpret_cast<const int32_t*>(tab + MT_PK);
  const float* pw = reinterpret_cast<const float*>(tab + MT_PW);
  float* db = dest + (int64_t)b * T * ldd;
  const int total = T * g.fw;
  constexpr int U = 4;  // as mel_stage: the loads of U elements first, then the arithmetic
  for (int base = threadIdx.x; base < total; base += 256 * U) {
    float re[U], im[U], o0[U], o1[U];
    int loc[U];
    int64_t off[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * 256;
      loc[u] = -1;
      re[u] = im[u] = o0[u] = o1[u] = 0.f;
      off[u] = 0;
      if (idx < total) {
        const int t = idx / g.fw, f = g.f_lo + (idx - t * g.fw);
        const int n = f * T + t;
        if (n >= g.n0 && n < g.n1) {
          loc[u] = n - g.n0;
          re[u] = eb[(int64_t)t * lde + f];
          im[u] = eb[(int64_t)t * lde + MEL_NB + f];
          off[u] = (int64_t)t * ldd + f;
          if (accumulate) {
            o0[u] = db[off[u]];
            o1[u] = db[off[u] + MEL_NB];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (loc[u] < 0) continue;
      const int row = loc[u] / MEL_NB, j = loc[u] - row * MEL_NB;
      float dm = 0.f;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int k = min(max(pk[j * 6 + i], 0), MEL_NF - 1);
        dm += av[row * MEL_NF + k] * pw[j * 6 + i];
      }
      const float k2 = dm / (512.0f * 512.0f * me[loc[u]]);
      db[off[u]] = o0[u] + k2 * re[u];
      db[off[u] + MEL_NB] = o1[u] + k2 * im[u];
    }
  }
}

}  // namespace clskd

using namespace clskd;

static int wave_check(const char* what, const float* s, int64_t lds, const float* y, int64_t ldy,
                      int32_t B, int32_t L) {
  CLSKD_CHECK_ARG(s && y, "%s: null pointer", what);
  CLSKD_CHECK_SHAPE(B >= 1 && B <= 65535 && L >= 1, "%s: B=%d (1..65535) L=%d", what, B, L);
  CLSKD_CHECK_SHAPE((B == 1 || (lds >= L && ldy >= L)), "%s: row strides %lld / %lld < L=%d", what,
                    (long long)lds, (long long)ldy, L);
  CLSKD_CHECK_ARG((((uintptr_t)s | (uintptr_t)y) & 3) == 0, "%s: s and y must be 4-byte aligned", what);
  return CLSKD_OK;
}

extern "C" int64_t clskd_wave_loss_workspace(int32_t B, int32_t L) {
  if (B < 1 || B > 65535 || L < 1) return 0;
  return (int64_t)B * wave_chunks(L) * 4 + (int64_t)B * 4;
}

extern "C" int clskd_wave_loss(const float* s, int64_t lds, const float* y, int64_t ldy, int32_t B,
                               int32_t L, const float* w5, float upstream, double* work,
                               float* out6, float* coef, void* stream) {
  const int rc = wave_check("wave_loss", s, lds, y, ldy, B, L);
  if (rc != CLSKD_OK) return rc;
  CLSKD_CHECK_ARG(w5 && work && out6, "wave_loss: null pointer");
  CLSKD_CHECK_ARG(((uintptr_t)work & 7) == 0, "wave_loss: work must be 8-byte aligned");
  CLSKD_CHECK_ARG((((uintptr_t)out6 | (uintptr_t)coef) & 3) == 0, "wave_loss: out / coef alignment");
  WaveW ww;
  for (int k = 0; k < 5; ++k) ww.w[k] = w5[k];
  hipStream_t st = as_stream(stream);
  const int nchunk = wave_chunks(L);
  double* rows = work + (int64_t)B * nchunk * 4;
  hipLaunchKernelGGL(wave_sums_kernel, dim3(nchunk, B), dim3(256), 0, st, s, lds, y, ldy, L, work);
  hipLaunchKernelGGL(wave_finalize_kernel, dim3(1), dim3(256), 0, st, work, nchunk, B, L, ww,
                     upstream, rows, out6, coef);
  CLSKD_LAUNCH_CHECK("wave_loss");
  return CLSKD_OK;
}

extern "C" int clskd_wave_loss_grad(const float* s, int64_t lds, const float* y, int64_t ldy,
                                    int32_t B, int32_t L, const float* coef, float* d_wav,
                                    int64_t ldd, int32_t accumulate, void* stream) {
  const int rc = wave_check("wave_loss_grad", s, lds, y, ldy, B, L);
  if (rc != CLSKD_OK) return rc;
  CLSKD_CHECK_ARG(coef && d_wav, "wave_loss_grad: null pointer");
  CLSKD_CHECK_SHAPE(B == 1 || ldd >= L, "wave_loss_grad: ldd=%lld < L=%d", (long long)ldd, L);
  CLSKD_CHECK_ARG((((uintptr_t)d_wav | (uintptr_t)coef) & 3) == 0, "wave_loss_grad: alignment");
  hipLaunchKernelGGL(wave_grad_kernel, dim3(wave_chunks(L), B), dim3(256), 0, as_stream(stream), s,
                     lds, y, ldy, L, coef, d_wav, ldd, accumulate);
  CLSKD_LAUNCH_CHECK("wave_loss_grad");
  return CLSKD_OK;
}

static int mel_check(const char* what, const float* clean, int32_t ldc, const float* est,
                     int32_t lde, int32_t B, int32_t T, const void* table) {
  CLSKD_CHECK_ARG(clean && est && table, "%s: null pointer", what);
  CLSKD_CHECK_SHAPE(B >= 1 && B <= 65535 && T >= 1 && T <= CLSKD_MEL_MAX_T,
                    "%s: B=%d (1..65535) T=%d (1..%d)", what, B, T, CLSKD_MEL_MAX_T);
  CLSKD_CHECK_SHAPE(ldc >= 514 && lde >= 514, "%s: ldc=%d lde=%d (< 514)", what, ldc, lde);
  CLSKD_CHECK_ARG((((uintptr_t)clean | (uintptr_t)est | (uintptr_t)table) & 3) == 0,
                  "%s: 4-byte alignment", what);
  return CLSKD_OK;
}

extern "C" int64_t clskd_mel_loss_workspace(int32_t B, int32_t T) {
  if (B < 1 || B > 65535 || T < 1 || T > CLSKD_MEL_MAX_T) return 0;
  return (int64_t)B * cdiv(T, MEL_ROWS);
}

extern "C" int clskd_mel_loss(const float* clean, int32_t ldc, const float* est, int32_t lde,
                              int32_t B, int32_t T, const void* table, double* work, float scale,
                              int32_t accumulate, float* out2, void* stream) {
  const int rc = mel_check("mel_loss", clean, ldc, est, lde, B, T, table);
  if (rc != CLSKD_OK) return rc;
  CLSKD_CHECK_ARG(work && out2, "mel_loss: null pointer");
  CLSKD_CHECK_ARG(((uintptr_t)work & 7) == 0, "mel_loss: work must be 8-byte aligned");
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mel_fwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)MEL_LDS_FWD);
    attr = true;
  }
  hipStream_t st = as_stream(stream);
  const int gx = (int)cdiv(T, MEL_ROWS);
  hipLaunchKernelGGL(mel_fwd_kernel, dim3(gx, B), dim3(256), MEL_LDS_FWD, st, clean, ldc, est, lde,
                     T, reinterpret_cast<const uint32_t*>(table), work);
  hipLaunchKernelGGL(mel_finalize_kernel, dim3(1), dim3(256), 0, st, work, (int64_t)B * gx,
                     3.0 * (double)B * (double)T, scale, accumulate, out2);
  CLSKD_LAUNCH_CHECK("mel_loss");
  return CLSKD_OK;
}

extern "C" int clskd_mel_loss_bwd(const float* clean, int32_t ldc, const float* est, int32_t lde,
                                  int32_t B, int32_t T, const void* table, float upstream,
                                  float* d_est, int32_t ldd, int32_t accumulate, void* stream) {
  const int rc = mel_check("mel_loss_bwd", clean, ldc, est, lde, B, T, table);
  if (rc != CLSKD_OK) return rc;
  CLSKD_CHECK_ARG(d_est && ((uintptr_t)d_est & 3) == 0, "mel_loss_bwd: null or misaligned d_est");
  CLSKD_CHECK_SHAPE(ldd >= 514, "mel_loss_bwd: ldd=%d (< 514)", ldd);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mel_bwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)MEL_LDS_BWD);
    attr = true;
  }
  const float gscale = (float)((double)upstream / (3.0 * (double)B * (double)T));
  hipLaunchKernelGGL(mel_bwd_kernel, dim3((unsigned)cdiv(T, MEL_ROWS), B), dim3(256), MEL_LDS_BWD,
                     as_stream(stream), clean, ldc, est, lde, T,
                     reinterpret_cast<const uint32_t*>(table), gscale, d_est, ldd, accumulate);
  CLSKD_LAUNCH_CHECK("mel_loss_bwd");
  return CLSKD_OK;
}
