// The convolution engines behind clskd_conv2d_fwd, each declared once.
//
// An engine's entry plans the descriptor once: *took says whether the layer is this engine's, and
// the planned launch goes out only when a stream is given (st == nullptr: decide only; no pointer
// of the descriptor is dereferenced).  The dispatcher, clskd_conv_fold_capable and
// clskd_conv_route all walk the one ordered table of these entries in conv_igemm.hip, so "would
// take" and "takes" are the same code.  A return other than CLSKD_OK refuses the descriptor (the
// error message is set).
#pragma once
#include "common.h"

namespace clskd {

typedef int (*ConvEntry)(const clskd_conv_desc& d, const hipStream_t* st, bool* took);

int conv_direct(const clskd_conv_desc& d, const hipStream_t* st, bool* took);      // conv_direct.hip
int conv_halo(const clskd_conv_desc& d, const hipStream_t* st, bool* took);        // conv_halo.hip
#ifdef CLSKD_EXPERIMENTS
int conv_halow(const clskd_conv_desc& d, const hipStream_t* st, bool* took);       // conv_halow.hip
#endif
int conv_gemm8(const clskd_conv_desc& d, const hipStream_t* st, bool* took);       // conv_gemm8.hip
int conv_lds_dma(const clskd_conv_desc& d, const hipStream_t* st, bool* took);     // conv_bf16.hip
int conv_pointwise(const clskd_conv_desc& d, const hipStream_t* st, bool* took);   // conv_pointwise.hip
int conv_halo_split(const clskd_conv_desc& d, const hipStream_t* st, bool* took);  // conv_halo_split.hip
int conv_split3(const clskd_conv_desc& d, const hipStream_t* st, bool* took);      // conv_split.hip
int conv_halo_f32(const clskd_conv_desc& d, const hipStream_t* st, bool* took);    // conv_halo32.hip
int conv_generic_f32(const clskd_conv_desc& d, const hipStream_t* st, bool* took);  // conv_igemm.hip

// K-tile visiting order of the gathering engines: channel-block-major (kt_taps x kt_cpt K-tiles:
// all taps of a bk-deep channel block, then the next block, so the rows a K-tile gathers were
// fetched by the previous one) when every K-tile lies inside one tap; otherwise the packed order
// (kt_taps = 1, kt_cpt = K / bk).  use_knob: the A/B switch CLSKD_G8_KORDER=0 (packed) applies.
inline void conv_k_order(const clskd_conv_desc& d, int bk, bool use_knob, int& kt_taps, int& kt_cpt) {
  kt_taps = 1;
  kt_cpt = d.K / bk;
  if ((!use_knob || knob(KNOB_G8_KORDER) != 0) && d.ntaps > 1 && d.ctot % bk == 0 &&
      (int64_t)d.ntaps * d.ctot == d.K) {
    kt_taps = d.ntaps;
    kt_cpt = d.ctot / bk;
  }
}

}  // namespace clskd
