// The frame the halo-tiled convolutions share (conv_halo.hip, conv_halo32.hip,
// conv_halo_split.hip, conv_halow.hip): persistent 512-thread workgroups walk a contiguous run of
// (batch, F-block, T-block) output tiles; per channel chunk the tile's input halo is staged once
// and read by every tap; BatchNorm statistics accumulate per workgroup in fp64.  Here: the
// geometry of that walk (host plan + kernel arguments), the tile cursor, the chunk table in LDS,
// the packed staging-slot word, and the closing statistics reduction.  What a kernel does with a
// staged chunk — its staging pipeline, MFMA loop and epilogue stores — stays in its own file.
#pragma once
#include "bnfold.h"
#include "common.h"

namespace clskd {

constexpr int HALO_MAXCH = 64;  // channel chunks a plan can hold (ctot <= 512 at 8 channels each)
constexpr int HALO_NTH = 512;   // threads per workgroup (8 waves), every halo kernel

// The part of a halo kernel's arguments that describes the walk.  A kernel's Args struct is
// { clskd_conv_desc d; HaloGeom g; <its own fields>; BnFoldArgs f; }.
struct HaloGeom {
  int32_t nchunk;
  int32_t chunk_seg[HALO_MAXCH];
  int32_t chunk_c0[HALO_MAXCH];    // channel offset inside the segment
  int32_t chunk_kofs[HALO_MAXCH];  // channel offset of the chunk inside one tap's ctot channels
  int32_t dfmin, dtmin;            // halo origin relative to (fo * stride_f, to)
  int32_t HF, HT, NPIX;            // halo extent (pixels) and count
  int32_t nfb, ntb, ntiles;        // tile grid: F-blocks, T-blocks, total
  int32_t nblk128;                 // statistics slots (ceil(M / 128))
  int32_t stats_ld;                // channels per statistics slot row (N; the full N of a
                                   // column-split launch whose stats pointer is pre-offset)
};

// ---- host: the shared part of a plan -----------------------------------------------------------
// Chunks of cw channels (tap-major K order: segments in order), the tap bounding box, the halo of
// an ft x tt output tile (HT rounded up to a multiple of ht_pad) and the tile grid.  false: the
// layer does not have the structure (the caller's engine path).  HF / HT <= 255: the slot word
// packs them in 8 bits.  Conditions of one kernel alone (dtype, alignment, LDS budget, staging
// instruction counts) are that kernel's *_plan.
inline bool halo_geom_plan(const clskd_conv_desc& d, int cw, int ft, int tt, int ht_pad,
                           int min_tiles, HaloGeom& g) {
  if (d.ntaps < 1 || d.ntaps > 16 || d.nseg > CLSKD_MAX_SEGS) return false;
  int nch = 0, kofs = 0;
  for (int s = 0; s < d.nseg; ++s) {
    if (d.seg_c[s] % cw) return false;
    if (d.seg[s].sB > INT32_MAX || d.seg[s].sF > INT32_MAX || d.seg[s].sT > INT32_MAX) return false;
    for (int c0 = 0; c0 < d.seg_c[s]; c0 += cw) {
      if (nch >= HALO_MAXCH) return false;
      g.chunk_seg[nch] = s;
      g.chunk_c0[nch] = c0;
      g.chunk_kofs[nch] = kofs + c0;
      ++nch;
    }
    kofs += d.seg_c[s];
  }
  if (kofs != d.ctot) return false;
  g.nchunk = nch;
  int dfmin = 1 << 20, dfmax = -(1 << 20), dtmin = 1 << 20, dtmax = -(1 << 20);
  for (int t = 0; t < d.ntaps; ++t) {
    dfmin = d.tap_df[t] < dfmin ? d.tap_df[t] : dfmin;
    dfmax = d.tap_df[t] > dfmax ? d.tap_df[t] : dfmax;
    dtmin = d.tap_dt[t] < dtmin ? d.tap_dt[t] : dtmin;
    dtmax = d.tap_dt[t] > dtmax ? d.tap_dt[t] : dtmax;
  }
  g.dfmin = dfmin;
  g.dtmin = dtmin;
  g.HF = (ft - 1) * d.stride_f + (dfmax - dfmin + 1);
  g.HT = (int)cdiv((tt - 1) + (dtmax - dtmin + 1), ht_pad) * ht_pad;
  if (g.HF > 255 || g.HT > 255) return false;
  g.NPIX = g.HF * g.HT;
  g.nfb = (int)cdiv(d.Fo, ft);
  g.ntb = (int)cdiv(d.To, tt);
  const int64_t nt = (int64_t)d.B * g.nfb * g.ntb;
  if (nt < min_tiles || nt > (1 << 30)) return false;
  g.ntiles = (int)nt;
  g.nblk128 = (int)cdiv((int64_t)d.B * d.Fo * d.To, 128);
  g.stats_ld = d.N;
  return true;
}

// halo pixel offset of tap t for output (0, 0) (0 past the last tap)
inline void halo_tap_pix(const clskd_conv_desc& d, const HaloGeom& g, int32_t out[16]) {
  for (int t = 0; t < 16; ++t)
    out[t] = t < d.ntaps ? (d.tap_df[t] - g.dfmin) * g.HT + (d.tap_dt[t] - g.dtmin) : 0;
}

// Layers with 32 < N <= 64 whose resident [64][K] weights do not fit LDS beside the halo buffers
// run as two 32-column launches: a[0] / a[1] are the plans of columns [0, 32) / [32, N).  Weights,
// bias, output columns and statistics of the second are offset by 32 (statistics rows keep the
// full N as leading dimension), and it is the one that finalizes a folded BatchNorm.  wsz / osz:
// bytes per weight / output element.
template <typename Args, typename Plan>
inline bool halo_halves_plan(const clskd_conv_desc& d, size_t wsz, size_t osz, Plan plan,
                             Args (&a)[2], size_t (&lds)[2]) {
  if (d.N <= 32 || d.N > 64 || d.nlo < d.N) return false;
  clskd_conv_desc d1 = d, d2 = d;
  d1.N = 32;
  d2.N = d.N - 32;
  d2.weight = reinterpret_cast<const char*>(d.weight) + (int64_t)32 * d.K * (int64_t)wsz;
  if (d.bias) d2.bias = d.bias + 32;
  d2.out = reinterpret_cast<char*>(d.out) + (int64_t)32 * d.oNlo * (int64_t)osz;
  if (d.stats) d2.stats = d.stats + 64;
  if (!plan(d1, a[0], lds[0]) || !plan(d2, a[1], lds[1])) return false;
  a[0].g.stats_ld = a[1].g.stats_ld = d.N;
  if (a[0].f.acc) {
    a[1].f = a[0].f;
    a[0].f.finalize = 0;
    a[1].f.c_off += 32;
  }
  return true;
}

// ---- tile cursor -------------------------------------------------------------------------------
// (b, fb, tb) of a tile, advanced incrementally: no divisions in a kernel's loop
struct HaloCursor {
  int b, fb, tb;
  __host__ __device__ __forceinline__ void advance(int nfb, int ntb) {
    if (++tb == ntb) {
      tb = 0;
      if (++fb == nfb) { fb = 0; ++b; }
    }
  }
};
__host__ __device__ __forceinline__ HaloCursor halo_cursor_of(int tile, int nfb, int ntb) {
  HaloCursor c;
  c.tb = tile % ntb;
  const int r = tile / ntb;
  c.fb = r % nfb;
  c.b = r / nfb;
  return c;
}

// ---- staging-slot word -------------------------------------------------------------------------
// A staging slot moves 16 B of halo pixel p: hf | ht << 8 | sub << 16 | valid << 20, where
// (hf, ht) is the pixel inside the halo and sub (< 16) the 16-B piece of its channel run that the
// slot reads (after the kernel's swizzle, for the LDS-DMA kernels).
__host__ __device__ __forceinline__ int halo_slot_pack(int p, int sub, bool ok, int HT) {
  const int pp = ok ? p : 0;
  const int hf = pp / HT, ht = pp - (pp / HT) * HT;
  return hf | (ht << 8) | (sub << 16) | ((ok ? 1 : 0) << 20);
}
// Source of a slot for the tile whose halo starts at input pixel (fi_lo, ti_lo) of an F x T
// segment: ok = the slot is valid and the pixel inside the segment (else it stages zeros).
struct HaloSlotSrc {
  int fi, ti, sub;
};
__host__ __device__ __forceinline__ HaloSlotSrc halo_slot_src(int word, int fi_lo, int ti_lo, int F,
                                                              int T, bool& ok) {
  HaloSlotSrc s;
  s.fi = fi_lo + (word & 0xff);
  s.ti = ti_lo + ((word >> 8) & 0xff);
  s.sub = (word >> 16) & 15;
  ok = ((word >> 20) & 1) && (unsigned)s.fi < (unsigned)F && (unsigned)s.ti < (unsigned)T;
  return s;
}

// ---- device ------------------------------------------------------------------------------------
// Kernel arguments are re-read by the compiler under SGPR pressure (s_load inside the loop),
// and scalar loads share lgkmcnt with LDS reads — every fragment wait then degrades to
// lgkmcnt(0).  Values the loop needs are therefore laundered through an opaque VGPR into an
// SGPR (no re-materialisation from the kernarg segment is possible) or staged in LDS.
__device__ __forceinline__ int sconst(int v) {
  asm volatile("" : "+v"(v));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int64_t vconst64(int64_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Chunk table in LDS, one entry per chunk: ctA {base lo, base hi, sF, sT}, ctB {sB, F, T, kofs}
// (base: the segment pointer advanced to the chunk's first channel; strides in elements).
__device__ __forceinline__ void halo_ctab_fill(int4* ctA, int4* ctB, const clskd_conv_desc& d,
                                               const HaloGeom& g, int elem_bytes) {
  const int tid = threadIdx.x;
  if (tid < g.nchunk) {
    const clskd_seg& S = d.seg[g.chunk_seg[tid]];
    const uint64_t base = (uint64_t)(uintptr_t)S.ptr + (uint64_t)((int64_t)g.chunk_c0[tid] * elem_bytes);
    ctA[tid] = make_int4((int)(unsigned)base, (int)(unsigned)(base >> 32), (int)S.sF, (int)S.sT);
    ctB[tid] = make_int4((int)S.sB, S.F, S.T, g.chunk_kofs[tid]);
  }
}
template <typename E>
struct HaloChunk {
  const E* base;  // of batch 0
  int sF, sT, sB, F, T, kofs;
};
template <typename E>
__device__ __forceinline__ HaloChunk<E> halo_chunk(const int4* ctA, const int4* ctB, int ch) {
  const int4 ea = ctA[ch];
  const int4 eb = ctB[ch];
  HaloChunk<E> c;
  c.base = reinterpret_cast<const E*>(((uint64_t)(unsigned)ea.y << 32) | (unsigned)ea.x);
  c.sF = ea.z;
  c.sT = ea.w;
  c.sB = eb.x;
  c.F = eb.y;
  c.T = eb.z;
  c.kofs = eb.w;
  return c;
}

// Partial-slot contract (include/clskd.h): workgroup b writes slot b; the slots past the grid are
// zeroed here, each workgroup its share.
__device__ __forceinline__ void halo_stats_zero_unowned(double* stats, int N, int stats_ld, int nblk128) {
  for (int64_t s = (int64_t)blockIdx.x + gridDim.x; s < nblk128; s += gridDim.x)
    for (int i = threadIdx.x; i < N * 2; i += HALO_NTH) stats[s * stats_ld * 2 + i] = 0.0;
}

// bias and output offset of this lane's column in each of NB 32-column blocks: launch columns
// [n0, n0 + N) of the descriptor's
template <int NB, bool LAUNDER>
__device__ __forceinline__ void halo_bias_coff(const clskd_conv_desc& d, int n0, int N, int l32,
                                               float (&bcol)[NB], int64_t (&coff)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = nb * 32 + l32;
    bcol[nb] = (d.bias && n < N) ? d.bias[n0 + n] : 0.f;
    const int64_t c = n < N ? conv_col_off(d, n0 + n) : -1;
    coff[nb] = LAUNDER ? vconst64(c) : c;
  }
}

// Workgroup partial of the statistics, called by every thread once the staging buffers at smem
// are free: the two lane halves by shuffle, then the NGROUP row groups (the waves) in
// a fixed order through red[NGROUP][BN][2] — bitwise reproducible.  st_s / st_q: this lane's
// NB column sums; col(nb): its column inside the BN of the workgroup; group: its row group.
// The result goes to the folded finalize (f.acc; f.c_off is the BatchNorm channel of column n0)
// or to partial slot blockIdx.x, as columns [n0, n0 + N) of a stats_ld-wide row.
template <int NGROUP, int BN, int NB, typename Col>
__device__ __forceinline__ void halo_stats_commit(const clskd_conv_desc& d, const BnFoldArgs& f,
                                                  unsigned char* smem, const double (&st_s)[NB],
                                                  const double (&st_q)[NB], int group, Col col,
                                                  int n0, int N, int stats_ld, int nblk128) {
  __syncthreads();
  double* red = reinterpret_cast<double*>(smem);
  const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const double s2 = st_s[nb] + __shfl_xor(st_s[nb], 32, 64);
    const double q2 = st_q[nb] + __shfl_xor(st_q[nb], 32, 64);
    if (h == 0) {
      red[(group * BN + col(nb)) * 2] = s2;
      red[(group * BN + col(nb)) * 2 + 1] = q2;
    }
  }
  __syncthreads();
  auto sum_groups = [&](int n, double& S, double& Q) {
    S = 0.0;
    Q = 0.0;
    for (int w = 0; w < NGROUP; ++w) {
      S += red[(w * BN + n) * 2];
      Q += red[(w * BN + n) * 2 + 1];
    }
  };
  if (f.acc) {
    bnfold_commit(f, N, sum_groups, reinterpret_cast<int*>(red + NGROUP * BN * 2), blockIdx.x,
                  gridDim.x);
  } else if (blockIdx.x < nblk128) {
    for (int n = threadIdx.x; n < N; n += HALO_NTH) {
      double S, Q;
      sum_groups(n, S, Q);
      d.stats[((int64_t)blockIdx.x * stats_ld + n0 + n) * 2] = S;
      d.stats[((int64_t)blockIdx.x * stats_ld + n0 + n) * 2 + 1] = Q;
    }
  }
}

}  // namespace clskd
