// Halo-tiled split-product convolution for the student's fp32 layers (16 <= N <= 64): the halo
// structure of conv_halo32.hip with the arithmetic of conv_split.hip (3 x bf16 split products,
// hi*W_hi + hi*W_lo + lo*W_hi into fp32 accumulators; tools_for_model.py:236-262, 303-330).
//
// conv_split3_kernel is an implicit GEMM over the im2col-expanded A operand: every input element
// is gathered and split once per tap that touches it (5 / 6 / 4 times for the 5x2 stride-2
// encoder layers and the decoder parities) and the weight matrix is re-read and re-split for
// every M-tile.  Here both happen once:
//   * persistent workgroups of 8 waves; output tile = 8 F-rows x 32 time steps (TW = 1), or
//     4 F-rows x 64 time steps (TW = 2) for layers with Fo <= 4, so all eight waves own one
//     32-row block of v_mfma_f32_32x32x16_bf16 either way;
//   * the input halo — ((8/TW - 1) * stride_f + F-taps) x (32*TW - 1 + T-taps) pixels — is read
//     once per channel chunk as 16-B pieces of each pixel's contiguous channel run, split once
//     (hi = bf16(x), lo = bf16(x - hi), RNE both) and kept in LDS as a hi and a lo plane; every
//     tap reads its A fragments from those planes (no K table, no per-tap address arithmetic:
//     the per-step LDS offsets are loop-invariant registers);
//   * the weights are split once per workgroup in the prologue and stay resident in LDS as hi /
//     lo planes in k-octet order [K/8][NBW][8 bf16]: the 32 lanes of a half read 512 contiguous
//     bytes (conflict-free).
//
// Staging: variant (a) of the two candidates — global loads into registers one chunk ahead,
// split, written to the other halo buffer after the current chunk's MFMAs (one barrier per
// chunk).  It is the pipeline conv_split3_kernel already has, with dense loads and one split per
// element; LDS-DMA (b) would land fp32 in LDS and need a second LDS pass (read fp32, write
// planes) plus an fp32 landing buffer twice the size of the planes it feeds.
//
// Channel chunks are CW = 16 channels (one tap per 16-deep MFMA step; 32-B plane rows, 16-B
// halves XOR-swizzled by (pixel >> 3) & 1 as in conv_split.hip) or CW = 8 (two taps per step:
// lanes 0-31 read tap a's pixel, lanes 32-63 tap b's; 16-B rows, contiguous; an odd tap count
// pads with a zero weight octet).  CW = 8 halves the halo buffers.
//
// LDS: 4 planes (2 buffers x hi / lo) of NPIX * 2 * CW bytes + 4 * NBW * (K + 8) bytes of
// weights + 2 KiB of tables, <= 160 KiB.  For the 5x2 stride-2 encoder tile NPIX = 19 x 33 = 627
// (TW = 2: 11 x 65 = 715), for the decoder parities 10 x 33 = 330 / 9 x 33 = 297 (TW = 2: 6 x 65
// / 5 x 65):
//   N = 32, K = 160 (CW 16): 78 + 21 KiB;   N = 64, K = 320 (CW 8): 39 + 82 KiB;
//   N = 64, K = 512 (CW 8): 19 + 130 KiB;   N = 32, K = 768 (CW 16): 41 + 97 KiB;
//   N = 64, K = 640 / 768: 160 / 194 KiB of weights do not fit — column halves: even / odd
//   workgroups of one launch keep the planes of columns [0, 32) / [32, N) resident (80 / 97 KiB)
//   and walk the same tiles; the halo is staged and split by both halves, the folded BatchNorm
//   finalize counts every workgroup of the launch (channel offset + 32 for the odd ones).
//
// The tile walk, the chunk table, the staging-slot word and the statistics reduction are
// conv_halo_common.h's; clskd_conv_halo_split_plan walks the staging loads with the same helpers.
#include <stdlib.h>

#include "conv_dispatch.h"
#include "conv_halo_common.h"

namespace clskd {

__device__ __attribute__((aligned(256))) unsigned char g_hs3_sink[4096];

typedef __attribute__((address_space(1))) float gfloat_hs3;

namespace hs3 {
typedef short s16x8 __attribute__((ext_vector_type(8)));
constexpr int NW = 8;       // waves (= 32-row MFMA blocks of a tile)
constexpr int NTH = HALO_NTH;
constexpr int MAXU = 6;     // 16-B staging loads per thread per chunk
constexpr int MAXCH = HALO_MAXCH;  // channel chunks (ctot <= 512 at CW = 8)
constexpr int MAXSTEP = 16; // 16-deep MFMA steps per chunk

// byte offset of k-quad q of pixel p inside a plane (CW 16: swizzled 16-B halves of 32-B rows)
__host__ __device__ inline int plane_off(int cw, int p, int q) {
  return cw == 16 ? p * 32 + ((((q >> 1) ^ (p >> 3)) & 1) << 4) + (q & 1) * 8 : p * 16 + (q & 1) * 8;
}

// Staging slot i of thread tid: k-quad q of halo pixel p.  Returns the slot word (sub = q) and
// the pixel whose plane offset the slot writes (0 for a slot past the halo: never written).
__host__ __device__ __forceinline__ int stage_slot(int tid, int i, int qp, int NU, int NPIX, int HT,
                                                   int& pp, int& q) {
  const int u = tid + i * NTH;
  const int p = u / qp;
  q = u % qp;
  const bool ok = i < NU && p < NPIX;
  pp = ok ? p : 0;
  return halo_slot_pack(p, q, ok, HT);
}
}  // namespace hs3

struct HaloSplitArgs {
  clskd_conv_desc d;
  HaloGeom g;
  int32_t cw, tw;                  // channels per chunk (8 | 16); 32-step T blocks per tile (1 | 2)
  int32_t NU;                      // staging loads per thread per chunk
  int32_t plane_bytes;             // bytes of one bf16 plane of the halo
  int32_t nstep;                   // 16-deep MFMA steps per chunk
  int32_t step_pix[2][hs3::MAXSTEP];  // halo pixel offset read by lane half h at step s
  int32_t step_oct[2][hs3::MAXSTEP];  // weight k-octet (chunk-relative; -1: the zero octet)
  int32_t koct;                    // k-octets of resident weights (ntaps * ctot / 8), + 1 zero octet
  int32_t nhalf;                   // 2: odd / even workgroups own output columns [0, 32) / [32, N)
  BnFoldArgs f;
};

template <int NB, int CW, int NSTEP>
__global__ __launch_bounds__(512) void conv_halo_split3_kernel(const HaloSplitArgs a) {
  using namespace hs3;
  const clskd_conv_desc& d = a.d;
  const HaloGeom& g = a.g;
  constexpr int NBW = NB * 32;
  constexpr int QP = CW / 4;           // 16-B staging loads per pixel
  constexpr int NACC = NB == 1 ? 3 : 1;  // NB = 1: the cross terms on accumulators of their own
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int plane_bytes = a.plane_bytes;
  unsigned char* hbuf = smem;                                   // [2 buffers][hi, lo][plane_bytes]
  unsigned char* wl = smem + 4 * plane_bytes;                   // [hi, lo][koct + 1][NBW][16 B]
  const int wplane = (a.koct + 1) * NBW * 16;
  int4* ctA = reinterpret_cast<int4*>(wl + 2 * wplane);         // [nchunk] {base lo, base hi, sF, sT}
  int4* ctB = ctA + MAXCH;                                      // [nchunk] {sB, F, T, kofs}

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, h = lane >> 5;
  // column halves (weights of all N columns do not fit): even / odd workgroups own columns
  // [0, 32) / [32, N) of the same tile list, each with its own resident weight planes
  const int nhalf = a.nhalf;
  const int half = nhalf == 2 ? (int)(blockIdx.x & 1) : 0;
  const int wgi = blockIdx.x / nhalf, nwg = gridDim.x / nhalf;
  const int n0 = half * 32;
  const int N = nhalf == 2 ? min(32, d.N - n0) : d.N;

  // ---- prologue: weights split once into resident hi / lo planes, chunk table, stats slots ----
  {
    const int64_t K = d.K;
    const float* wg = reinterpret_cast<const float*>(d.weight) + n0 * K;
    const int total = a.koct * NBW * 2;  // k-quads
    constexpr int WB = 8;  // independent 16-B loads in flight per thread before the splits
    const int kq2 = a.koct * 2;  // k-quads per weight row: consecutive threads read one row
    for (int base = tid; base < total; base += NTH * WB) {
      f32x4 v[WB];
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = base + j * NTH;
        const int n = idx / kq2, kq = idx - n * kq2;
        v[j] = (idx < total && n < N) ? *reinterpret_cast<const f32x4*>(wg + n * K + kq * 4)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = base + j * NTH;
        if (idx < total) {
          const int n = idx / kq2, kq = idx - n * kq2;
          s16x4 hi, lo;
          split4(v[j], hi, lo);
          const int off = ((kq >> 1) * NBW + n) * 16 + (kq & 1) * 8;
          *reinterpret_cast<s16x4*>(wl + off) = hi;
          *reinterpret_cast<s16x4*>(wl + wplane + off) = lo;
        }
      }
    }
    for (int i = tid; i < NBW * 4; i += NTH) {  // the zero octet of both planes
      const int pl = i / (NBW * 2), piece = i - pl * NBW * 2;
      *reinterpret_cast<int2*>(wl + pl * wplane + a.koct * NBW * 16 + piece * 8) = make_int2(0, 0);
    }
  }
  halo_ctab_fill(ctA, ctB, d, g, 4);
  if (d.stats) {  // slots no workgroup owns (grid <= nblk128) are zero
    halo_stats_zero_unowned(d.stats, d.N, g.stats_ld, g.nblk128);
    if (nhalf == 2)  // the other half's columns of this workgroup's own slot
      for (int i = tid; i < (d.N - N) * 2; i += NTH)
        d.stats[((int64_t)blockIdx.x * g.stats_ld + (half ? 0 : 32)) * 2 + i] = 0.0;
  }
  float bcol[NB];
  int64_t coff[NB];
  halo_bias_coff<NB, false>(d, n0, N, l32, bcol, coff);
  const int nchunk = g.nchunk, ntb = g.ntb, nfb = g.nfb, NU = a.NU;
  const int tw = a.tw, FT = NW / tw, TT = 32 * tw;
  const int Fo = d.Fo, To = d.To, sfr = d.stride_f;
  const int dfmin = g.dfmin, dtmin = g.dtmin;
  const int64_t oB = d.oB, oF = d.oF, oT = d.oT;
  const int of_mul = d.of_mul, of_add = d.of_add;
  gfloat_hs3* const outp = reinterpret_cast<gfloat_hs3*>((uintptr_t)d.out);
  // per-thread staging slots: the slot word (sub = k-quad) and the LDS offset it writes
  int ug[MAXU], uo[MAXU];
  {
    const int HT = g.HT, NPIX = g.NPIX;
#pragma unroll
    for (int i = 0; i < MAXU; ++i) {
      int pp, q;
      ug[i] = stage_slot(tid, i, QP, NU, NPIX, HT, pp, q);
      uo[i] = plane_off(CW, pp, q);
    }
  }
  // per-step fragment offsets of this lane (loop-invariant): A inside a halo plane, B inside a
  // weight plane (bit 31: the zero octet, no chunk offset added)
  const int frow = wave / tw, tblk = wave - frow * tw;
  int sa[NSTEP];
  unsigned sb[NSTEP];
  {
    const int prow0 = frow * sfr * g.HT + tblk * 32 + l32;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      const int p = prow0 + (h ? a.step_pix[1][s] : a.step_pix[0][s]);
      const int oct = h ? a.step_oct[1][s] : a.step_oct[0][s];
      sa[s] = CW == 16 ? p * 32 + (((h ^ (p >> 3)) & 1) << 4) : p * 16;
      sb[s] = oct < 0 ? (0x80000000u | (unsigned)((a.koct * NBW + l32) * 16))
                      : (unsigned)((oct * NBW + l32) * 16);
    }
  }
  __syncthreads();

  const int per = (g.ntiles + nwg - 1) / nwg;
  const int tile_begin = wgi * per;
  const int ntile_blk = max(0, min(g.ntiles, tile_begin + per) - tile_begin);

  f32x4 ra[MAXU];
  // global loads of one chunk's halo into registers: out-of-range pixels are zero (a select,
  // never a load)
  auto load_chunk = [&](const HaloCursor& c, int ch) {
    const HaloChunk<float> k = halo_chunk<float>(ctA, ctB, ch);
    const float* base = k.base + (int64_t)c.b * k.sB;
    const int fi_lo = c.fb * FT * sfr + dfmin, ti_lo = c.tb * TT + dtmin;
#pragma unroll
    for (int i = 0; i < MAXU; ++i) {
      if (i < NU) {
        bool ok;
        const HaloSlotSrc s = halo_slot_src(ug[i], fi_lo, ti_lo, k.F, k.T, ok);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4*>(base + (int64_t)s.fi * k.sF + (int64_t)s.ti * k.sT + s.sub * 4);
        ra[i] = v;
      }
    }
  };
  auto store_chunk = [&](int buf) {
    unsigned char* hb = hbuf + buf * 2 * plane_bytes;
#pragma unroll
    for (int i = 0; i < MAXU; ++i) {
      if (i < NU && ((ug[i] >> 20) & 1)) {
        s16x4 hi, lo;
        split4(ra[i], hi, lo);
        *reinterpret_cast<s16x4*>(hb + uo[i]) = hi;
        *reinterpret_cast<s16x4*>(hb + plane_bytes + uo[i]) = lo;
      }
    }
  };

  f32x16 acc[NACC][NB];
  double st_s[NB], st_q[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) st_s[nb] = st_q[nb] = 0.0;

  // chunk stream over this workgroup's tiles: chunk it computes from buffer it & 1 while chunk
  // it + 1 (loaded one round ago) is split into the other buffer and chunk it + 2 is loaded
  const int total = ntile_blk * nchunk;
  HaloCursor cur = halo_cursor_of(tile_begin, nfb, ntb), nxt = cur;
  int nxt_ch = 0;
  auto step_next = [&]() {
    if (++nxt_ch == nchunk) { nxt_ch = 0; nxt.advance(nfb, ntb); }
  };
  if (total > 0) {
    load_chunk(nxt, nxt_ch);
    step_next();
    store_chunk(0);
    if (total > 1) {
      load_chunk(nxt, nxt_ch);
      step_next();
    }
  }
  __syncthreads();

  int it = 0;
  for (int ti = 0; ti < ntile_blk; ++ti) {
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][nb][r] = q == 0 ? bcol[nb] : 0.f;
    for (int ch = 0; ch < nchunk; ++ch, ++it) {
      const unsigned char* hb = hbuf + (it & 1) * 2 * plane_bytes;
      const unsigned kofsb = (unsigned)((ctB[ch].w >> 3) * NBW * 16);
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        const s16x8 ahi = *reinterpret_cast<const s16x8*>(hb + sa[s]);
        const s16x8 alo = *reinterpret_cast<const s16x8*>(hb + plane_bytes + sa[s]);
        const unsigned bo = (sb[s] & 0x7fffffffu) + ((sb[s] >> 31) ? 0u : kofsb);
        s16x8 bhi[NB], blo[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          bhi[nb] = *reinterpret_cast<const s16x8*>(wl + bo + nb * 512);
          blo[nb] = *reinterpret_cast<const s16x8*>(wl + wplane + bo + nb * 512);
        }
        if constexpr (NB == 1) {  // three chains: no back-to-back dependent MFMA
          acc[0][0] = mfma16<__bf16>(ahi, bhi[0], acc[0][0]);
          acc[1][0] = mfma16<__bf16>(alo, bhi[0], acc[1][0]);
          acc[2][0] = mfma16<__bf16>(ahi, blo[0], acc[2][0]);
        } else {  // the column blocks alternate
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[0][nb] = mfma16<__bf16>(ahi, bhi[nb], acc[0][nb]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[0][nb] = mfma16<__bf16>(alo, bhi[nb], acc[0][nb]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[0][nb] = mfma16<__bf16>(ahi, blo[nb], acc[0][nb]);
        }
      }
      if (it + 1 < total) store_chunk((it + 1) & 1);
      if (it + 2 < total) {
        load_chunk(nxt, nxt_ch);
        step_next();
      }
      __syncthreads();
    }
    // ---- tile epilogue: statistics and a static number of stores (invalid rows: sink page) ---
    const int fo = cur.fb * FT + frow;
    const int to0 = cur.tb * TT + tblk * 32;
    const int64_t obase = (int64_t)cur.b * oB + (int64_t)(fo * of_mul + of_add) * oF + (int64_t)to0 * oT;
    gfloat_hs3* sink = reinterpret_cast<gfloat_hs3*>((uintptr_t)g_hs3_sink) + lane;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const bool nok = coff[nb] >= 0;
      float sm = 0.f, sq = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // MFMA C row = output time offset
        const bool ok = nok && fo < Fo && to0 + row < To;
        float v = acc[0][nb][r];
#pragma unroll
        for (int q = 1; q < NACC; ++q) v += acc[q][nb][r];
        if (ok) {
          sm += v;
          sq = fmaf(v, v, sq);
        }
        gfloat_hs3* dst = ok ? outp + obase + (int64_t)row * oT + coff[nb] : sink;
        *dst = v;
      }
      st_s[nb] += (double)sm;
      st_q[nb] += (double)sq;
    }
    cur.advance(nfb, ntb);
  }

  if (d.stats || a.f.acc) {  // workgroup partial: red[NW][NBW][2] over the halo buffers
    BnFoldArgs f = a.f;
    f.c_off += n0;
    halo_stats_commit<NW, NBW>(d, f, smem, st_s, st_q, wave, [&](int nb) { return nb * 32 + l32; }, n0, N,
                               g.stats_ld, g.nblk128);
  }
}

// Routing rule, per layer class on measurement (tools/conv_micro.py --student, B = 16, T = 643,
// isolated µs per launch, conv_split3_kernel -> this kernel, spreads 0.5-4 µs;
// profiles/halo_split_micro.txt):
//   N = 64 encoder (enc3)                82 -> 40      N = 32 (enc2, dec2 parities)  41 -> 33, 86 -> 49, 62 -> 42
//   N = 64 decoder parity (dec1 p1)      61 -> 44      N = 16 (dec3 parities)        81 -> 57, 60 -> 51
//   Fo = 4 (enc5, dec0 parities)         49 -> 33, 56 -> 35, 42 -> 28
//   column halves (enc4, dec1 p0; and enc5, dec0 p0 above)   72 -> 47, 83 -> 47
// every class is taken.  Two separate 32-column launches measured 66 (enc4) and 66 (dec1 p0): the
// halves share one launch instead.  N = 8 (dec4 parity 0, K = 192) measured 101 against 91: the
// epilogue stores 32-B row pieces and three quarters of the MFMA columns are zero — N < 16 stays
// on conv_split3_kernel.  Spanning only 128 CUs (CLSKD_HALO_SPLIT_GRID=128) measured -0.03 ms in
// the concurrent step (5.10 against 5.13 ms) but loses to conv_split3_kernel in isolation on four
// classes (e.g. enc2 44 against 40): not adopted, the grid spans every CU.
//
// Plan + eligibility (host).  false: not this kernel (conv_split3_kernel runs the layer).
static bool halo_split_plan1(const clskd_conv_desc& d, HaloSplitArgs& a, size_t& lds, int cw) {
  using namespace hs3;
  if (d.in_dtype != CLSKD_F32 || d.compute != CLSKD_F32 || d.out_dtype != CLSKD_F32) return false;
  if (d.accumulate || d.wlayout != CLSKD_WLAYOUT_NK) return false;
  if (d.N < 16 || d.N > 64 || d.stride_t != 1) return false;
  if (d.stride_f < 1 || d.stride_f > 2 || d.ctot < cw || d.ctot % cw) return false;
  if (d.nseg < 1 || d.nseg > CLSKD_MAX_SEGS) return false;
  a.d = d;
  a.cw = cw;
  for (int s = 0; s < d.nseg; ++s) {  // 16-B loads of every segment's channel runs
    const clskd_seg& g = d.seg[s];
    if (d.seg_c[s] < cw) return false;
    if (((uintptr_t)g.ptr & 15) || g.sB % 4 || g.sF % 4 || g.sT % 4) return false;
    if (g.sB < 0 || g.sF < 0 || g.sT < 0) return false;
  }
  a.tw = d.Fo <= 4 ? 2 : 1;  // 4 F-rows x 64 steps: all eight waves work on a 4-row layer
  if (!halo_geom_plan(d, cw, NW / a.tw, 32 * a.tw, 1, 32, a.g)) return false;
  if (d.ntaps * d.ctot > d.K || d.K % 8) return false;
  if (((uintptr_t)d.weight & 15)) return false;
  a.NU = (int)cdiv((int64_t)a.g.NPIX * (cw / 4), NTH);
  if (a.NU > MAXU) return false;
  a.plane_bytes = (a.g.NPIX * cw * 2 + 15) & ~15;
  a.koct = d.ntaps * d.ctot / 8;
  a.nstep = cw == 16 ? d.ntaps : (d.ntaps + 1) / 2;
  if (a.nstep > MAXSTEP) return false;
  int32_t tap_pix[16];
  halo_tap_pix(d, a.g, tap_pix);
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < MAXSTEP; ++s) {
      // CW 16: both lane halves read tap s (channel octets 0 / 1 of the chunk); CW 8: taps 2s, 2s+1
      const int t = cw == 16 ? s : 2 * s + h;
      const bool on = s < a.nstep && t < d.ntaps;
      a.step_pix[h][s] = on ? tap_pix[t] : 0;
      a.step_oct[h][s] = on ? t * (d.ctot / 8) + (cw == 16 ? h : 0) : -1;
    }
  const int NBW = d.N <= 32 ? 32 : 64;
  lds = 4 * (size_t)a.plane_bytes + 2 * (size_t)(a.koct + 1) * NBW * 16 + 2 * MAXCH * 16;
  if (lds > 160 * 1024) return false;
  if ((size_t)NW * NBW * 16 + 16 > 4 * (size_t)a.plane_bytes) return false;  // statistics scratch
  a.nhalf = 1;
  a.f = make_bnfold(d);
  return true;
}

// 16-channel chunks (half the chunk rounds per tile) where the segments allow them and the
// buffers fit, else 8-channel chunks
static bool halo_split_plan(const clskd_conv_desc& d, HaloSplitArgs& a, size_t& lds) {
  return halo_split_plan1(d, a, lds, 16) || halo_split_plan1(d, a, lds, 8);
}

static bool halo_split_built(const HaloSplitArgs& a) {
  const int n = a.nstep;
  return a.cw == 16 ? (n == 4 || n == 6 || n == 9 || n == 10) : (n == 2 || n == 3 || n == 5);
}

// Every condition under which the layer is not this kernel's (conv_split3_kernel runs it): the
// knob, the plan, a built tap count.  When the [64][K] weight planes do not fit beside the halo
// buffers the launch runs as two column halves (nhalf = 2): even / odd workgroups keep the weight
// planes of columns [0, 32) / [32, N) resident and walk the same tile list — one launch, one
// prologue per workgroup; the halo is staged and split by both halves.  (The grid is cut to the
// statistics slots, halo_split_grid: no statistics condition declines.)
static bool halo_split_decide(const clskd_conv_desc& d, HaloSplitArgs& a, size_t& lds) {
  if (knob(KNOB_HALO_SPLIT) != 1) return false;
  if (!halo_split_plan(d, a, lds)) {
    if (d.N <= 32 || d.N > 64) return false;
    clskd_conv_desc d1 = d, d2 = d;
    d1.N = 32;
    d2.N = d.N - 32;
    HaloSplitArgs a2;
    size_t lds2 = 0;
    if (!halo_split_plan(d2, a2, lds2) || !halo_split_plan(d1, a, lds)) return false;
    if (a2.cw != a.cw || lds2 != lds) return false;  // (same geometry: never)
    a.d = d;
    a.g.stats_ld = d.N;
    a.nhalf = 2;
  }
  return halo_split_built(a);  // not a built tap count: conv_split3_kernel
}

static int halo_split_grid(const HaloSplitArgs& a) {
  const int ncu = device_cu_count();
  // CLSKD_SPLIT_GRID caps the CUs the grid spans (tests: many tiles per workgroup)
  const int gcap = knob(KNOB_SPLIT_GRID);
  int cus = gcap > 0 && gcap < ncu ? gcap : ncu;
  const int own = knob(KNOB_HALO_SPLIT_GRID);  // this kernel's own span (0: every CU)
  if (own > 0 && own < cus) cus = own;
  int nwg = cus / a.nhalf;
  nwg = a.g.ntiles < nwg ? a.g.ntiles : nwg;
  if (a.d.stats && nwg * a.nhalf > a.g.nblk128) nwg = a.g.nblk128 / a.nhalf;  // a statistics slot each
  return (nwg > 0 ? nwg : 1) * a.nhalf;
}

static void launch_halo_split_planned(const HaloSplitArgs& a, size_t lds, hipStream_t st) {
  const int grid = halo_split_grid(a);
#define HS3_LAUNCH(NB_, CW_, NS_)                                                              \
  do {                                                                                         \
    auto k = conv_halo_split3_kernel<NB_, CW_, NS_>;                                           \
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                              160 * 1024);                                                     \
    hipLaunchKernelGGL(k, dim3(grid), dim3(512), lds, st, a);                                  \
    note_kernel_fn((const void*)k);                                                            \
    note_kernel("conv_halo_split3_kernel<%d,%d,%d>", NB_, CW_, NS_);                           \
  } while (0)
#define HS3_NB(CW_, NS_)                                                                       \
  do {                                                                                         \
    if (a.d.N <= 32 || a.nhalf == 2) HS3_LAUNCH(1, CW_, NS_); else HS3_LAUNCH(2, CW_, NS_);                    \
  } while (0)
  if (a.cw == 16) {
    switch (a.nstep) {
      case 4: HS3_NB(16, 4); break;
      case 6: HS3_NB(16, 6); break;
      case 9: HS3_NB(16, 9); break;
      default: HS3_NB(16, 10); break;
    }
  } else {
    switch (a.nstep) {
      case 2: HS3_NB(8, 2); break;
      case 3: HS3_NB(8, 3); break;
      default: HS3_NB(8, 5); break;
    }
  }
#undef HS3_NB
#undef HS3_LAUNCH
}

int conv_halo_split(const clskd_conv_desc& d, const hipStream_t* st, bool* took) {
  HaloSplitArgs a;
  size_t lds = 0;
  *took = halo_split_decide(d, a, lds);
  if (*took && st) launch_halo_split_planned(a, lds, *st);
  return CLSKD_OK;
}

}  // namespace clskd

// The plan of a descriptor, for checking before anything runs: the tile grid, the halo, the LDS
// footprint and — by walking every tile, chunk and staging slot with the kernel's own index
// arithmetic (the cursor and slot helpers the kernel uses) — the smallest and largest element
// offset the staging loads touch per segment.
extern "C" int clskd_conv_halo_split_plan(const clskd_conv_desc* dp, clskd_halo_split_info* info) {
  using namespace clskd;
  using namespace clskd::hs3;
  CLSKD_CHECK_ARG(dp && info, "halo_split_plan: null argument");
  memset(info, 0, sizeof(*info));
  clskd_conv_desc d = *dp;
  if (d.compute == CLSKD_F32X3) d.compute = CLSKD_F32;
  HaloSplitArgs p;
  size_t lds = 0;
  if (!halo_split_decide(d, p, lds)) return CLSKD_OK;
  const HaloGeom& g = p.g;
  const int QP = p.cw / 4, FT = NW / p.tw, TT = 32 * p.tw;
  info->launches = 1;
  info->col_halves = p.nhalf;
  info->cw = p.cw;
  info->tile_f = FT;
  info->tile_t = TT;
  info->nfb = g.nfb;
  info->ntb = g.ntb;
  info->ntiles = g.ntiles;
  info->halo_f = g.HF;
  info->halo_t = g.HT;
  info->nchunk = g.nchunk;
  info->nstep = p.nstep;
  info->lds_bytes = (int64_t)lds;
  info->grid = halo_split_grid(p);
  for (int s = 0; s < CLSKD_MAX_SEGS; ++s) {
    info->seg_min_off[s] = INT64_MAX;
    info->seg_max_off[s] = INT64_MIN;
  }
  for (int s = 0; s < p.nstep; ++s)
    for (int h = 0; h < 2; ++h) {  // the farthest fragment read stays inside the plane
      const int pmax = (FT - 1) * p.d.stride_f * g.HT + (p.tw - 1) * 32 + 31 + p.step_pix[h][s];
      CLSKD_CHECK_ARG(pmax < g.NPIX, "halo_split_plan: fragment pixel %d outside the halo %d", pmax, g.NPIX);
    }
  int ug[MAXU * NTH];  // the slot words of every thread, as the kernel packs them
  for (int i = 0; i < MAXU; ++i)
    for (int tid = 0; tid < NTH; ++tid) {
      int pp, q;
      ug[i * NTH + tid] = stage_slot(tid, i, QP, p.NU, g.NPIX, g.HT, pp, q);
    }
  HaloCursor c = halo_cursor_of(0, g.nfb, g.ntb);
  for (int tile = 0; tile < g.ntiles; ++tile, c.advance(g.nfb, g.ntb)) {
    const int fi_lo = c.fb * FT * p.d.stride_f + g.dfmin, ti_lo = c.tb * TT + g.dtmin;
    for (int ch = 0; ch < g.nchunk; ++ch) {
      const int sg = g.chunk_seg[ch];
      const clskd_seg& S = p.d.seg[sg];
      for (int u = 0; u < p.NU * NTH; ++u) {
        bool ok;
        const HaloSlotSrc s = halo_slot_src(ug[u], fi_lo, ti_lo, S.F, S.T, ok);
        if (!ok) continue;
        const int64_t off = g.chunk_c0[ch] + (int64_t)c.b * S.sB + (int64_t)s.fi * S.sF + (int64_t)s.ti * S.sT + s.sub * 4;
        if (off < info->seg_min_off[sg]) info->seg_min_off[sg] = off;
        if (off + 3 > info->seg_max_off[sg]) info->seg_max_off[sg] = off + 3;
      }
    }
  }
  return CLSKD_OK;
}
