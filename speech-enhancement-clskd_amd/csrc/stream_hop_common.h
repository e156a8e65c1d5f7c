// Layer machinery shared by the fused streaming-hop kernels (stream_hop.hip: the DCCRN student,
// stream_hop_mini.hip: asteroid's DCCRNet_mini): one 512-thread workgroup per stream, the current
// frame of each layer in LDS, weights in k-quad layout [K/4][N][4] straight from L2 into
// registers (`pipeline`), split-K convolution layers over an LDS window (`conv` / `conv_layer`,
// `Geo` / `xrow`) and the dense rows (`gemv`).  A kernel that wants phase timestamps defines
// CMARK(i) before including this header; otherwise the marks compile to nothing.
#pragma once
#include "common.h"

#ifndef CMARK
#define CMARK(i) \
  do {           \
  } while (0)
#endif

namespace clskd {
namespace shop {

constexpr int NT = 512;    // threads per stream workgroup (8 waves: two per SIMD)
constexpr int HOP = 100, WIN = 400, NBIN = 514, LDEST = 516;
constexpr int WINSZ = 4096;      // conv input window [2][F][Ci] ...
constexpr int ZOFF = WINSZ;      // ... followed by a zero row (out-of-range taps read it)
constexpr int RED = NT * 16;     // split-K partial sums (threads x R x CQ)

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int ring(int f, int D) { return ((f % D) + D) % D; }
// log2 of a power of two (every shape the layer helpers divide by is one: host-checked)
__device__ __forceinline__ int lg2(int v) { return 31 - __builtin_clz(v); }

// The layer helpers below are out-of-line (one copy of each in the code object: the whole hop
// inlined was 121 KB of straight-line code, refetched from L2 by the instruction cache every hop),
// so their pointers carry explicit address spaces: LDS operands as `lds`, global ones cast to
// `gbl` — a generic pointer would turn every access into a flat one (counted on both vmcnt and
// lgkmcnt, which serialises the weight prefetch).
typedef __attribute__((address_space(3))) float lds;
typedef __attribute__((address_space(1))) const float gbl;
typedef __attribute__((address_space(3))) const f32x4 lds4;
typedef __attribute__((address_space(1))) const f32x4 gbl4;
__device__ __forceinline__ f32x4 ld4(const lds* p) { return *(lds4*)p; }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ldg4(const float* p) { return *(gbl4*)p; }
__device__ __forceinline__ float ldg(const float* p) { return *(gbl*)p; }
__device__ __forceinline__ lds* L(float* p) { return (lds*)p; }
__device__ __forceinline__ const lds* L(const float* p) { return (const lds*)p; }
__device__ __forceinline__ void fma4(f32x2& acc, const f32x4 w, const f32x4 x) {
  acc = __builtin_elementwise_fma(w.xy, x.xy, acc);
  acc = __builtin_elementwise_fma(w.zw, x.zw, acc);
}

// Weight quads stream from global memory straight into registers, QB float4 per lane per batch
// (KB quads x CQ channels) and NB batches deep: batch b's loads issue NB - 1 batches before it
// computes, and the first NB - 1 batches issue before the layer stages its input (`pre`), so the
// staging round trip and the first weight round trip overlap.  Trip counts are uniform and the
// loads unconditional (indices clamped to the matrix; quads past a slice's end meet the zero row
// instead), so the compiler keeps the batches in flight with counted vmcnt waits.  NB = 3 ran
// the same hop time as NB = 2 (131.6 vs 131.2 us) with 256 VGPRs and spills, so NB = 2.
constexpr int QB = 8, NB = 2;

template <class T, class Load, class Comp, class Pre>
__device__ __forceinline__ void pipeline(int nbat, T (&buf)[NB], Load&& load, Comp&& comp, Pre&& pre) {
#pragma unroll
  for (int u = 0; u < NB - 1; ++u)
    if (u < nbat) load(buf[u], u);
  pre();
  for (int b0 = 0; b0 < nbat; b0 += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int bt = b0 + u;
      if (bt < nbat) {
        if (bt + NB - 1 < nbat) load(buf[(u + NB - 1) % NB], bt + NB - 1);
        comp(buf[u], bt);
      }
    }
  }
}

// Convolution geometry of one layer over the LDS window win [2][F][Ci] (slot 1 = newest frame).
// Tap j: encoder (kf = j/2, kt = j%2) reads row fo*2 + kf - 2 of slot kt; decoder (per parity,
// _DEC_TAPS in model.py) reads row fo + 1 - j/2 of slot 1 - j%2.
struct Geo {
  int F, Ci, lgq, sf, dec;  // lgq = log2(Ci / 4)
};
// (bitwise selects: a conditional expression here became exec-masked branches per row)
__device__ __forceinline__ int pick(bool c, int a, int b) {
  const int m = -(int)c;
  return (a & m) | (b & ~m);
}
__device__ __forceinline__ int xrow(const Geo& g, int j, int fo, bool live = true) {
  const int tdf = g.dec ? 1 - (j >> 1) : (j >> 1) - 2;
  const int tsl = g.dec ? 1 - (j & 1) : (j & 1);
  const int fi = fo * g.sf + tdf;
  return pick(live && (unsigned)fi < (unsigned)g.F, (tsl * g.F + fi) << (g.lgq + 2), ZOFF);
}

// out[(fo*of_mul + p)*Co + co] = act(bias_p[co] + sum_k W_p[k][co] x_p(fo, k)) for fo < Fo and
// each of np parities p (W_p: K4_p quads, k-quad layout); coef: BN [scale | shift] + PReLU.
// Thread = (parity, K slice ks, row group fg, channel group cg): R rows fo = fg + FG*r times CQ
// channels co = cg*CQ + q, so each activation quad (an LDS broadcast) feeds CQ channels and each
// weight quad R rows.  S K-slices per output fill the block; partials reduce through `red`
// (np*S*Fo*Co <= NT*R*CQ floats).  PERTAP: taps narrower than a batch (Ci < 4*KB), window
// offsets per quad; else per batch (slices start on whole batches, so one tap per batch).
// stage(): fills win (called with the first weight batches in flight; a barrier follows), here
// also the bias / BN / PReLU parameters go to `prm` (np*Co + 2*Co + 2 floats).
// Requires FG*(Co/CQ)*S a multiple of 64 (the parity is wave-uniform).  Uniform across the block.
// REIM: two PReLU slopes, alpha[0] for channels [0, Co/2) (real) and alpha[1] for [Co/2, Co)
// (imaginary): asteroid's OnReIm(PReLU).
template <int R, int CQ, bool PERTAP, bool REIM, class Stage>
__device__ __forceinline__ void conv(const lds* win, const Geo g, int np, int K4a, int K4b, int Fo, int Co,
                                     const float* W0, const float* W1, const float* b0, const float* b1,
                                     const float* coef, const float* alpha, lds* out, int of_mul, lds* red,
                                     lds* prm, int mk, Stage&& stage) {
  constexpr int KB = QB / CQ / (PERTAP ? 2 : 1);  // per-quad offsets cost registers
  constexpr int LR = R == 8 ? 3 : 2, LQ = CQ == 2 ? 1 : 0;
  const int tid = threadIdx.x;
  // every count is a power of two: shifts and masks, no integer divisions
  const int lfo = lg2(Fo), lco = lg2(Co);
  const int lfg = lfo - LR, lcg = lco - LQ;
  const int FG = 1 << lfg, CG = 1 << lcg;
  const int ls = max(0, lg2(NT) - (np == 2 ? 1 : 0) - lfg - lcg);
  const int S = 1 << ls;
  const int lp = lfg + lcg + ls;
  const int p = __builtin_amdgcn_readfirstlane(tid >> lp);
  const int rem = tid & ((1 << lp) - 1);
  const int cg = rem & (CG - 1), fg = (rem >> lcg) & (FG - 1), ks = rem >> (lcg + lfg);
  const bool act = p < np;
  const int pc = act ? p : 0;
  const int k4n = pc ? K4b : K4a;
  int len = (k4n + S - 1) >> ls;
  len = (len + KB - 1) / KB * KB;
  const int nbat = __builtin_amdgcn_readfirstlane(act ? len / KB : 0);
  const int k0 = ks * len, k1 = min(k4n, k0 + len);
  const float* W = (pc ? W1 : W0) + cg * CQ * 4;
  const int stride = Co * 4;
  const int qm = (1 << g.lgq) - 1;
  f32x2 acc[R][CQ];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int q = 0; q < CQ; ++q) acc[r][q] = f32x2{0.f, 0.f};
  struct Batch {
    f32x4 w[KB][CQ];
  };
  Batch buf[NB];
  pipeline(
      nbat, buf,
      [&](Batch& bb, int bt) {
        const int kb = k0 + bt * KB;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          const float* src = W + (size_t)min(kb + i, k4n - 1) * stride;
#pragma unroll
          for (int q = 0; q < CQ; ++q) bb.w[i][q] = ldg4(src + q * 4);
        }
      },
      [&](const Batch& bb, int bt) {
        const int kb = k0 + bt * KB;
        int off[R];
        if (!PERTAP) {
          const int j = kb >> g.lgq;
#pragma unroll
          for (int r = 0; r < R; ++r) off[r] = xrow(g, j, fg + FG * r, kb < k1);
        }
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          const int k4 = kb + i;
          if (PERTAP) {
            const int j = k4 >> g.lgq;
#pragma unroll
            for (int r = 0; r < R; ++r) off[r] = xrow(g, j, fg + FG * r, k4 < k1);
          }
          const int c = (k4 & qm) << 2;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const f32x4 x = ld4(win + off[r] + c);
#pragma unroll
            for (int q = 0; q < CQ; ++q) fma4(acc[r][q], bb.w[i][q], x);
          }
        }
      },
      [&]() {
        stage();
        for (int q = tid; q < np * Co; q += NT) {
          const float* bp = q >= Co ? b1 : b0;
          prm[q] = bp ? ldg(bp + (q & (Co - 1))) : 0.f;
        }
        if (coef) {
          for (int q = tid; q < 2 * Co; q += NT) prm[np * Co + q] = ldg(coef + q);
          if (tid < (REIM ? 2 : 1)) prm[np * Co + 2 * Co + tid] = ldg(alpha + tid);
        }
        __syncthreads();
      });
  if (mk >= 0) __syncthreads();
  CMARK(mk);
  auto fin = [&](int pp, int fo, int cc, float v) {
    v += prm[pp * Co + cc];
    if (coef) {
      v = fmaf(v, prm[np * Co + cc], prm[np * Co + Co + cc]);
      v = v >= 0.f ? v : prm[np * Co + 2 * Co + (REIM ? (int)(cc >= (Co >> 1)) : 0)] * v;
    }
    out[(fo * of_mul + pp) * Co + cc] = v;
  };
  if (S == 1) {
    if (act)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < CQ; ++q) fin(p, fg + FG * r, cg * CQ + q, acc[r][q].x + acc[r][q].y);
    return;
  }
  if (act)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < CQ; ++q)
        red[((p * S + ks) * Fo + fg + FG * r) * Co + cg * CQ + q] = acc[r][q].x + acc[r][q].y;
  __syncthreads();
  CMARK(mk < 0 ? -1 : mk + 1);
  for (int q = tid; q < (np << (lfo + lco)); q += NT) {
    const int pp = q >> (lfo + lco), o = q & ((1 << (lfo + lco)) - 1);
    float v = 0.f;
    for (int s2 = 0; s2 < S; ++s2) v += red[(((pp << ls) + s2) << (lfo + lco)) + o];
    fin(pp, o >> lco, o & (Co - 1), v);
  }
}

// One layer: R = min(Fo, 8) rows and CQ = 2 channels per thread where Co >= 16.  zero: the
// layer's output frame is out of range (staging still runs).
template <bool REIM = false, class Stage>
__device__ __forceinline__ void conv_layer(const lds* win, const Geo g, int np, int K4a, int K4b, int Fo, int Co,
                                           const float* W0, const float* W1, const float* b0, const float* b1,
                                           const float* coef, const float* alpha, lds* out, int of_mul,
                                           lds* red, lds* prm, bool zero, int mk, Stage&& stage) {
  if (zero) {
    stage();
    const int lfc = lg2(Fo) + lg2(Co);
    for (int q = threadIdx.x; q < (np << lfc); q += NT) {
      const int p = q >> lfc, o = q & ((1 << lfc) - 1);
      out[((o >> lg2(Co)) * of_mul + p) * Co + (o & (Co - 1))] = 0.f;
    }
    return;
  }
#define CONV_ARGS win, g, np, K4a, K4b, Fo, Co, W0, W1, b0, b1, coef, alpha, out, of_mul, red, prm, mk, stage
  if (Fo >= 8) {
    if (Co >= 16) {
      if (g.Ci < 16) conv<8, 2, true, REIM>(CONV_ARGS);  // (CQ = 2: KB = 4 quads, a tap of Ci >= 16 spans >= 4)
      else conv<8, 2, false, REIM>(CONV_ARGS);
    } else {
      if (g.Ci < 4 * QB) conv<8, 1, true, REIM>(CONV_ARGS);
      else conv<8, 1, false, REIM>(CONV_ARGS);
    }
  } else {
    // Fo == 4 (host-checked): encoder 5 and decoder 0 of the student, Ci >= 16 and Co >= 16
    conv<4, 2, false, REIM>(CONV_ARGS);
  }
#undef CONV_ARGS
}

// y[h*ys + n] = bias[n] + sum_k W[k][n] x[h*xs + k] for n < N, h < nh; W in k-quad layout with
// K4 quads, x in LDS (16-B aligned rows).  Units (K slice, h, n) over the block, rounds of NT
// units with uniform trip counts (idle units compute on clamped indices and do not store);
// with S > 1 slices the partials reduce through `red`.  pre(): stages x (called with the first
// weight batches of round 0 in flight; a barrier follows).  The caller synchronises before
// reading y.
template <class Pre>
__device__ __forceinline__ void gemv(const float* W, const float* bias, const lds* x, int xs, int nh, int K4, int N,
                                     lds* y, int ys, lds* red, const lds* zrow, Pre&& pre) {
  const int tid = threadIdx.x;
  const int M = nh * N;
  // K slices: the least work per thread over rounds of NT units, a round costing its quads
  // plus ~8 quads of fixed work (unit indices, partial store, the pipeline's first round trip);
  // ties: fewer slices.  (Counting quads alone picked 14 rounds of 8 quads for the STFT row.)
  int S = 1, best = 1 << 30;
  for (int s2 = 1; s2 <= 16 && s2 * M <= RED && s2 <= K4; ++s2) {
    const int cost = (s2 * M + NT - 1) / NT * ((K4 + s2 - 1) / s2 + 8);
    if (cost < best) {
      best = cost;
      S = s2;
    }
  }
  const int len = (K4 + S - 1) / S;
  const int nbat = __builtin_amdgcn_readfirstlane((len + QB - 1) / QB);
  const int U = S * M;
  struct Batch {
    f32x4 w[QB];
  };
  for (int u0 = 0; u0 < U; u0 += NT) {
    const int u = min(u0 + tid, U - 1);
    const int ks = u / M, hn = u - ks * M, h = hn / N, n = hn - h * N;
    const lds* xr = x + h * xs;
    const float* Wn = W + n * 4;
    const int k0 = ks * len, k1 = min(K4, k0 + len);
    f32x2 acc = f32x2{0.f, 0.f};
    Batch buf[NB];
    pipeline(
        nbat, buf,
        [&](Batch& bb, int bt) {
#pragma unroll
          for (int i = 0; i < QB; ++i) bb.w[i] = ldg4(Wn + (size_t)min(k0 + bt * QB + i, K4 - 1) * N * 4);
        },
        [&](const Batch& bb, int bt) {
          const int kb = k0 + bt * QB;
#pragma unroll
          for (int i = 0; i < QB; ++i) fma4(acc, bb.w[i], ld4(kb + i < k1 ? xr + (kb + i) * 4 : zrow));
        },
        [&]() {
          if (u0 == 0) {
            pre();
            __syncthreads();
          }
        });
    if (u0 + tid < U) {
      if (S == 1)
        y[h * ys + n] = acc.x + acc.y + (bias ? ldg(bias + n) : 0.f);
      else
        red[u] = acc.x + acc.y;
    }
  }
  if (S == 1) return;
  __syncthreads();
  for (int q = tid; q < M; q += NT) {
    float v = bias ? ldg(bias + q % N) : 0.f;
    for (int s2 = 0; s2 < S; ++s2) v += red[s2 * M + q];
    y[(q / N) * ys + q % N] = v;
  }
}


// The two complex-LSTM layers of a hop (nn.LSTM gates i, f, g, o; the four evaluations R(r), I(i),
// R(i), I(r) of a layer in one pass; gates as clskd_lstm_cell), (h, c) carried across hops in
// hs / cs [layer][ws][half][H] (global).  Inlined: one call site per hop kernel.
// LDS scratch, 16-byte aligned where read as quads: xin [2][K] the staged input halves (layer 0:
// x[k = f*Ch + c] = enc5[f][half*Ch + c] with K = D4*Ch, layer 1: the combine output, K = H),
// gx [2][8*64] (gate inputs, both weight sets side by side), hv / cv [2][2][64], act [2][2][4*64],
// whh [2*4H][H + 4] (rows padded by 4 floats: the gate loop's row-per-lane quad reads are
// conflict-free), red / zr as gemv.  cur: encoder 5's frame [D4][C6] (LDS); e5ring: the slot of
// encoder 5's ring that receives it (written behind the first weight loads).  rin: the layer
// output, [re | im] rows of rs floats — the next layer's input and the caller's projection
// operand.  w / b / whh_g: the args' lstm_w / lstm_b / lstm_whh.  Block-uniform; ends on a barrier.
struct LstmLds {
  lds *xin, *gx, *hv, *cv, *act, *whh, *rin, *red;
  const lds *zr, *cur;
};
__device__ __forceinline__ void lstm_hop(const LstmLds s, int rs, float* e5ring, const float* const* w,
                                         const float* const* b, const float* const* whh_g, float* hs0,
                                         float* cs0, int H, int D4, int C6) {
  const int tid = threadIdx.x;
  const int Ch = C6 / 2, G4 = 4 * H;
  for (int li = 0; li < 2; ++li) {
    const int K = li == 0 ? D4 * Ch : H;
    float* hs = hs0 + li * 4 * H;  // [ws][half][H]
    float* cs = cs0 + li * 4 * H;
    // gate q = (ws, half, g), W_hh row n = ws*4H + g
    const bool gate = tid < 4 * G4;
    const int lh = lg2(H), lg4 = lh + 2;  // G4 = 4H
    const int q = gate ? tid : 0, ws = q >> (lg4 + 1), half = (q >> lg4) & 1, gg = q & (G4 - 1), n = ws * G4 + gg;
    gemv(w[li], b[li], s.xin, K, 2, K / 4, 8 * H, s.gx, 8 * 64, s.red, s.zr, [&]() {
      if (li == 0)
        for (int q2 = tid; q2 < D4 * C6; q2 += NT) e5ring[q2] = s.cur[q2];
      for (int q2 = tid; q2 < (H / 4) * 2 * G4; q2 += NT) {
        const int j4 = q2 >> (lg4 + 1), r = q2 & (2 * G4 - 1);
        *(__attribute__((address_space(3))) f32x4*)&s.whh[r * (H + 4) + j4 * 4] = ldg4(whh_g[li] + (size_t)q2 * 4);
      }
      for (int q2 = tid; q2 < 2 * K; q2 += NT) {
        const int lk = lg2(K), lch = lg2(Ch);
        const int half2 = q2 >> lk, k = q2 & (K - 1);
        s.xin[q2] = li == 0 ? s.cur[(k >> lch) * C6 + half2 * Ch + (k & (Ch - 1))] : s.rin[half2 * rs + k];
      }
      for (int q2 = tid; q2 < 4 * H; q2 += NT) {
        s.hv[(q2 >> lh) * 64 + (q2 & (H - 1))] = hs[q2];
        s.cv[(q2 >> lh) * 64 + (q2 & (H - 1))] = cs[q2];
      }
    });
    __syncthreads();
    // a = gx + W_hh[ws][g] . h[ws][half]
    if (gate) {
      f32x2 s2 = f32x2{s.gx[half * 8 * 64 + n], 0.f};
      for (int j4 = 0; j4 < H / 4; ++j4)
        fma4(s2, ld4(&s.whh[n * (H + 4) + j4 * 4]), ld4(&s.hv[(ws * 2 + half) * 64 + j4 * 4]));
      const float a = s2.x + s2.y;
      s.act[(ws * 2 + half) * 4 * 64 + gg] = (gg >> lh) == 2 ? tanh_gate(a) : sigm_fast(a);
    }
    __syncthreads();
    for (int q2 = tid; q2 < 4 * H; q2 += NT) {
      const int wh = q2 >> lh, u = q2 & (H - 1);
      const lds* ac = s.act + wh * 4 * 64;
      const float cn = ac[H + u] * s.cv[wh * 64 + u] + ac[u] * ac[2 * H + u];
      const float hn = ac[3 * H + u] * tanh_fast(cn);
      cs[q2] = cn;
      hs[q2] = hn;
      s.hv[wh * 64 + u] = hn;
    }
    __syncthreads();
    // real = R(r) - I(i), imag = R(i) + I(r)  (tools_for_model.py:168-169)
    for (int q2 = tid; q2 < 2 * H; q2 += NT) {
      const int half2 = q2 >> lh, u = q2 & (H - 1);
      s.rin[half2 * rs + u] = half2 == 0 ? s.hv[u] - s.hv[3 * 64 + u] : s.hv[64 + u] + s.hv[2 * 64 + u];
    }
    __syncthreads();
    CMARK(8 + li);
  }
}

}  // namespace shop
}  // namespace clskd
