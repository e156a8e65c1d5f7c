// What the implicit-GEMM convolution engines (conv_igemm.hip, conv_bf16.hip, conv_split.hip,
// conv_gemm8.hip) share beyond common.h: the packed K-chunk word, its decode and the table fill,
// and the LDS-DMA engines' zero page.  Every other piece of their common frame (row table, tile
// deal, statistics, scatter epilogue) stays per kernel: its shared form cost some instance
// registers or time (profiles/gemm_common_codegen.txt).
#pragma once
#include "common.h"

namespace clskd {

// what an out-of-bounds tap of the LDS-DMA engines reads (one per translation unit that uses it)
static __device__ __attribute__((aligned(64))) unsigned char gemm_zero_page[64];

// ---- K-chunk table -----------------------------------------------------------------------------
// One entry per Q consecutive k (Q = 4 fp32 or 8 16-bit values: 16 B of one tap and segment):
// x = element offset, y = dF (16 bits, signed) | dT (8 bits, signed) << 16 | segment << 24.
struct KChunk {
  int off, dF, dT, seg;
};
__host__ __device__ __forceinline__ int2 kchunk_pack(const clskd_ktab_entry& e, int seg) {
  return make_int2(e.off, (int)(((unsigned)e.dF & 0xFFFFu) | (((unsigned)e.dT & 0xFFu) << 16) |
                                ((unsigned)seg << 24)));
}
__host__ __device__ __forceinline__ KChunk kchunk_decode(const int2 ce) {
  KChunk c;
  c.off = ce.x;
  c.dF = (int)(short)(ce.y & 0xFFFF);
  c.dT = (int)(signed char)((ce.y >> 16) & 0xFF);
  c.seg = (int)((unsigned)ce.y >> 24);
  return c;
}
template <int Q>
__device__ __forceinline__ void gemm_ctab_fill(int2* ctab, const clskd_conv_desc& d, int tid, int nthreads) {
  static_assert(Q == 4 || Q == 8, "k per chunk entry");
  for (int q = tid; q < d.K / Q; q += nthreads) ctab[q] = kchunk_pack(d.ktab[q * Q], d.kseg[q * Q]);
}

}  // namespace clskd
