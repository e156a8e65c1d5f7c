// One streaming hop of asteroid's DCCRNet_mini ('DCCRN-CL-test', clskd/asteroid.py) as ONE kernel
// launch: the model the reference distils and evaluates, at the widths of the C5 student, so the
// layer machinery of stream_hop.hip (stream_hop_common.h) applies unchanged — one 512-thread
// workgroup per stream, the current frame of every layer in LDS, older frames in per-stream
// global rings that only earlier launches wrote, weights in k-quad layout [K/4][N][4] straight
// into registers, split-K, both transposed-conv parities in one pass.  fp32 throughout,
// BatchNorm in eval mode (running statistics: the only mode in which this model is streamable).
//
// Time structure (oracle/asteroid_cpu.py:85-138).  Hop h brings samples [100h, 100h+100); frame u
// covers [100u, 100u+400) (no centring), so the newest complete frame of hop h is u = h - 3.
// Encoder i looks AHEAD (5x2 kernel, no time padding: output frame t reads input frames t, t+1),
// so at frame u it emits its frame u-(i+1); the LSTMs (carried h, c), the Linear and the six
// causal transposed convs (output frame t reads input frames t, t-1) emit frame u-6; the mask of
// frame u-6 multiplies spectrum frame u-6, and the synthesis frame enters a 4-frame plain
// overlap-add whose 100 final samples are block u-6 = h-9 of the offline output.
//
// Frames that the offline forward does not have must be ZERO wherever a later layer reads them
// (BatchNorm + PReLU of a zero row is not zero, and the output layer has a bias), so every
// layer's frame is forced to zero when it does not exist: a spectrum frame u < 0 or (drain)
// u >= T; encoder i's frame u-i-1 < 0 or while draining; the LSTM / Linear frame u-6 < 0 or
// while draining (their state is then left untouched); transposed conv d (0..5) emits frame u-6
// only for u >= 6 and, in drain hop k = u-T+1 >= 1, only while k <= d+1 (its output has T-5+d
// frames).
//
// Ring slots: frame f of a ring of depth D lives in slot ((f % D) + D) % D; rings start zeroed.
// Depths: spectrum 7 (frames u-6 .. u), encoder output i: 7-i (it writes frame u-i-1, the skip of
// transposed conv 5-i reads u-6 and u-7), transposed-conv inputs 2 (u-6, u-7), synthesis 4.
#include "stream_hop_common.h"

namespace clskd {

__global__ __launch_bounds__(shop::NT) void stream_hop_mini_kernel(const clskd_stream_hop_mini_args a) {
  using namespace shop;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int u = a.t - 3;     // newest spectrum frame
  const int u6 = u - 6;      // frame of the LSTM, the transposed convs, the mask and the output
  const int kd = a.drain;    // 0 on a live hop, else the drain hop 1 ..
  const bool spec_ok = a.live && u >= 0;
  const bool lstm_ok = a.live && u6 >= 0;
  float* st = a.state + (int64_t)b * a.state_stride;
  const int H = a.H, D4 = a.D4, C6 = a.enc_cout[5], Ch = C6 / 2;

  __shared__ __attribute__((aligned(16))) float xw[WIN];
  __shared__ __attribute__((aligned(16))) float spec[NBIN + 2];
  __shared__ __attribute__((aligned(16))) float win[WINSZ + 256];
  __shared__ __attribute__((aligned(16))) float curA[1024];
  __shared__ __attribute__((aligned(16))) float curB[1024];  // ping-pong: current frame of a layer
  __shared__ __attribute__((aligned(16))) float decin[256];
  __shared__ __attribute__((aligned(16))) float gx[2][8 * 64];
  __shared__ __attribute__((aligned(16))) float hv[2][2][64];
  __shared__ __attribute__((aligned(16))) float cv[2][2][64];
  __shared__ __attribute__((aligned(16))) float act[2][2][4 * 64];
  __shared__ __attribute__((aligned(16))) float rin[2 * 64];  // [re H | im H] (the Linear's K)
  __shared__ __attribute__((aligned(16))) float est[LDEST];
  __shared__ __attribute__((aligned(16))) float frame[WIN];
  __shared__ __attribute__((aligned(16))) float red[RED];
  __shared__ __attribute__((aligned(16))) float prm[512];
  __shared__ __attribute__((aligned(16))) float whh[8 * 32 * 36];  // W_hh [2*4H][H + 4], H <= 32

  for (int i = tid; i < 256; i += NT) win[ZOFF + i] = 0.f;
  const float* zr = win + ZOFF;  // zero row (LDS)
  // ---- input window: shift by one hop, append the new samples (zeros on a drain hop)
  float* gxw = st + a.off_xwin;
  auto stage_x = [&]() {
    for (int i = tid; i < WIN; i += NT)
      xw[i] = i < WIN - HOP ? gxw[i + HOP] : (a.live ? a.x_in[(int64_t)b * HOP + i - (WIN - HOP)] : 0.f);
  };

  float* cur = curA;
  float* nxt = curB;
  // ---- STFTFB analysis row of the newest window (asteroid.py:301-304); no frame yet / any more: 0
  if (spec_ok) {
    gemv(a.stft_w, nullptr, L(xw), 0, 1, WIN / 4, NBIN, L(spec), 0, L(red), L(zr), stage_x);
  } else {
    stage_x();
    for (int i = tid; i < NBIN + 2; i += NT) spec[i] = 0.f;
  }
  __syncthreads();
  // ---- encoders (asteroid.py:309-320): window [u-i-1, u-i] of the input, taps (kf - 2, kt),
  //      stride 2 in F, no bias.  The ring writes of the previous phase's output are issued in
  //      the next phase's staging, behind its first weight loads (stream_hop.hip).
  for (int i = 0; i < 6; ++i) {
    const int Fi = 256 >> i, Fo = Fi / 2, Co = a.enc_cout[i];
    const int Ci = i == 0 ? 4 : a.enc_cin[i];  // encoder 0: (re, im) padded to a quad
    auto stage = [&]() {
      if (i == 0) {
        for (int j = tid; j < WIN; j += NT) gxw[j] = xw[j];  // (every read of gxw is behind a barrier)
        float* sring = st + a.off_spec;
        for (int j = tid; j < NBIN; j += NT) sring[ring(u, 7) * NBIN + j] = spec[j];
        const float* sp = st + a.off_spec + ring(u - 1, 7) * NBIN;
        for (int q = tid; q < 4 * Fi; q += NT) {  // bins 0 .. 255: the Nyquist bin is dropped
          const int f = q >> 2, ri = q & 3;
          win[q] = ri < 2 ? sp[(ri ? 257 : 0) + f] : 0.f;
          win[4 * Fi + q] = ri < 2 ? spec[(ri ? 257 : 0) + f] : 0.f;
        }
      } else {
        const int D = 7 - (i - 1);
        float* ep = st + a.off_enc[i - 1];
        const float* rp = ep + (int64_t)ring(u - i - 1, D) * Fi * Ci;
        float* er = ep + (int64_t)ring(u - i, D) * Fi * Ci;  // encoder i-1's frame u-i (this hop's)
        for (int q = tid; q < Fi * Ci; q += NT) {
          win[q] = rp[q];
          win[Fi * Ci + q] = cur[q];
          er[q] = cur[q];
        }
      }
    };
    const Geo g{Fi, Ci, 31 - __builtin_clz(Ci / 4), 2, 0};
    const bool none = !(a.live && u >= i + 1);
    conv_layer<true>(L(win), g, 1, 10 * Ci / 4, 0, Fo, Co, a.enc_w[i], nullptr, nullptr, nullptr, a.enc_coef[i],
                     a.enc_alpha[i], L(nxt), 1, L(red), L(prm), none, -1, stage);
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  // cur = encoder 5's frame u-6: [D4][C6]
  float* e5r = st + a.off_enc[5] + (int64_t)ring(u6, 2) * D4 * C6;
  if (lstm_ok) {
    // ---- two complex LSTM layers (asteroid.py:328-344): nn.LSTM gates i, f, g, o, the four
    //      evaluations R(r), I(i), R(i), I(r) of a layer in one pass, (h, c) carried across hops
    lstm_hop(LstmLds{L(win), L(&gx[0][0]), L(&hv[0][0][0]), L(&cv[0][0][0]), L(&act[0][0][0]), L(whh),
                     L(rin), L(red), L(zr), L(cur)},
             H, e5r, a.lstm_w, a.lstm_b, a.lstm_whh, st + a.off_h, st + a.off_c, H, D4, C6);
    // ---- complex Linear with bias, no residual (asteroid.py:345-350): K = (re H | im H),
    //      n = half*P + c*D4 + f -> dec_in[f][half*Ch + c]
    float* pj = &act[0][0][0];  // [2][Ch*D4] (the gate scratch is free now)
    gemv(a.lin_w, a.lin_b, L(rin), 0, 1, 2 * H / 4, 2 * Ch * D4, L(pj), 0, L(red), L(zr), []() {});
    __syncthreads();
    for (int q = tid; q < 2 * Ch * D4; q += NT) {
      const int ld4 = lg2(D4), lcd = lg2(Ch) + ld4;
      const int half = q >> lcd, n = q & ((1 << lcd) - 1);
      decin[(n & (D4 - 1)) * C6 + half * Ch + (n >> ld4)] = pj[q];
    }
    __syncthreads();
  } else {
    // no LSTM frame: encoder 5's frame (zeros) -> its ring, the decoder input is absent (zero)
    for (int q = tid; q < D4 * C6; q += NT) {
      e5r[q] = cur[q];
      decin[q] = 0.f;
    }
    __syncthreads();
  }

  // ---- transposed convs (asteroid.py:352-373; d = 5 is the output layer, with bias and without
  //      BatchNorm): layer d emits frame u-6 from frames [u-7, u-6] of its input and of encoder
  //      5-d's output; both parities in one pass
  const float* in_cur = decin;  // frame u-6 of this layer's input
  for (int d = 0; d < 6; ++d) {
    const int F = D4 << d, Ca = a.dec_ca[d], Cb = a.dec_cb[d], Ci = Ca + Cb, Co = a.dec_co[d];
    const int ie = 5 - d, De = 7 - ie;
    const bool dead = !(u6 >= 0 && kd <= d + 1);
    const float* in_old = d == 0 ? st + a.off_decin + ring(u6 - 1, 2) * D4 * C6
                                 : st + a.off_dout[d - 1] + (int64_t)ring(u6 - 1, 2) * F * Ca;
    const float* sk_old = st + a.off_enc[ie] + (int64_t)ring(u6 - 1, De) * F * Cb;
    const float* sk_new = d == 0 ? cur : st + a.off_enc[ie] + (int64_t)ring(u6, De) * F * Cb;
    const bool last = d == 5;
    // _DEC_TAPS (asteroid.py): parity 0 -> dF (1, 0, -1), parity 1 -> dF (1, 0); K order per tap
    // (kt = 0, 1) with window slot 1 - kt (kt = 0 reads frame u-6, kt = 1 frame u-7)
    const Geo g{F, Ci, 31 - __builtin_clz(Ci / 4), 1, 1};
    conv_layer<true>(L(win), g, 2, 6 * Ci / 4, 4 * Ci / 4, F, Co, a.dec_w[d][0], a.dec_w[d][1], a.dec_b[d][0],
                     a.dec_b[d][1], last ? nullptr : a.dec_coef[d], last ? nullptr : a.dec_alpha[d], L(nxt), 2,
                     L(red), L(prm), dead, -1, [&]() {
                       // the previous phase's output -> its ring (behind this layer's first weight loads)
                       if (d == 0) {
                         float* dr = st + a.off_decin + ring(u6, 2) * D4 * C6;
                         for (int q = tid; q < D4 * C6; q += NT) dr[q] = decin[q];
                       } else {  // layer d-1's frame u-6: [2 F_{d-1} = F][Co_{d-1} = Ca]
                         float* orr = st + a.off_dout[d - 1] + (int64_t)ring(u6, 2) * F * Ca;
                         for (int q = tid; q < F * Ca; q += NT) orr[q] = in_cur[q];
                       }
                       const int lci = g.lgq + 2;
                       for (int q = tid; q < F * Ci; q += NT) {
                         const int f = q >> lci, c = q & (Ci - 1);
                         win[q] = c < Ca ? in_old[f * Ca + c] : sk_old[f * Cb + c - Ca];
                         win[F * Ci + q] = c < Ca ? in_cur[f * Ca + c] : sk_new[f * Cb + c - Ca];
                       }
                     });
    __syncthreads();
    in_cur = nxt;
    // ping-pong: the next layer writes the other buffer (cur holds encoder 5 only for d == 0)
    nxt = (nxt == curA) ? curB : curA;
  }
  // in_cur = mask of frame u-6: [256][2] (re, im)
  // ---- BoundComplexMask('tanh') times the spectrum of frame u-6 on bins 0 .. 255, Nyquist 0
  //      (clskd_mask_bdt's arithmetic; staged while the first synthesis weight batches load),
  //      STFTFB synthesis row, plain overlap-add
  const float* s6 = st + a.off_spec + ring(u6, 7) * NBIN;
  gemv(a.istft_w, nullptr, L(est), 0, 1, LDEST / 4, WIN, L(frame), 0, L(red), L(zr), [&]() {
    for (int f = tid; f < 257; f += NT) {
      float er = 0.f, ei = 0.f;
      if (f < 256) {
        const float mr = in_cur[f * 2], mi = in_cur[f * 2 + 1];
        const float mag = tanhf(hypotf(mr, mi));
        const float ph = atan2f(mi, mr);
        const float br = mag * cosf(ph), bi = mag * sinf(ph);
        const float xr = s6[f], xi = s6[257 + f];
        er = br * xr - bi * xi;
        ei = br * xi + bi * xr;
      }
      est[f] = er;
      est[257 + f] = ei;
    }
    if (tid < 2) est[514 + tid] = 0.f;
  });
  __syncthreads();
  float* fr = st + a.off_frames;
  for (int i = tid; i < WIN; i += NT) fr[ring(u6, 4) * WIN + i] = frame[i];
  // block u-6 of the output: samples 300 + n of frame u-9, 200 + n of u-8, 100 + n of u-7, n of u-6
  for (int n = tid; n < HOP; n += NT) {
    float acc = 0.f;
    for (int k = 0; k < 4; ++k) {
      const int o = n + 300 - k * HOP;
      acc += k == 3 ? frame[o] : fr[ring(u6 - 3 + k, 4) * WIN + o];
    }
    a.wav_out[(int64_t)b * HOP + n] = acc;
  }
}

}  // namespace clskd

using namespace clskd;

extern "C" int clskd_stream_hop_mini(const clskd_stream_hop_mini_args* a, void* stream) {
  CLSKD_CHECK_ARG(a && a->state && a->wav_out && a->stft_w && a->istft_w && a->lin_w && a->lin_b,
                  "stream_hop_mini: null argument");
  CLSKD_CHECK_ARG(!a->live || a->x_in, "stream_hop_mini: live hop without input");
  CLSKD_CHECK_SHAPE(a->B >= 1 && a->t >= 0 && a->drain >= 0 && (a->live != 0) == (a->drain == 0),
                    "stream_hop_mini: B=%d t=%d live=%d drain=%d (a hop is live or a drain hop >= 1)", a->B, a->t,
                    a->live, a->drain);
  auto pow2 = [](int v) { return v >= 1 && (v & (v - 1)) == 0; };
  CLSKD_CHECK_SHAPE(a->H >= 4 && pow2(a->H) && a->H <= 32 && 16 * a->H <= shop::NT && a->D4 >= 1 &&
                        pow2(a->D4) && a->D4 * a->enc_cout[5] <= 256 && a->enc_cout[5] % 2 == 0,
                    "stream_hop_mini: H=%d D4=%d outside the built LDS budget", a->H, a->D4);
  CLSKD_CHECK_SHAPE(a->enc_cin[0] == 2, "stream_hop_mini: encoder 0 takes (re, im), got %d", a->enc_cin[0]);
  // conv_layer's thread plans (stream_hop_common.h): R = 8 rows (4 where Fo == 4), CQ = 2 channels
  // where Co >= 16 (or Fo == 4); the plan's (rows / R) * (Co / CQ) per parity must fit the block.
  auto plan_ok = [&](int Fo, int Co, int Ci, int np) {
    const int R = Fo >= 8 ? 8 : 4, CQ = (Fo < 8 || Co >= 16) ? 2 : 1;
    return pow2(Fo) && Fo >= 4 && (Fo >= 8 || (Co >= 16 && Ci >= 16)) && np * (Fo / R) * (Co / CQ) <= shop::NT &&
           Co % CQ == 0;
  };
  for (int i = 0; i < 6; ++i) {
    const int Fi = 256 >> i, Fo = Fi / 2, Co = a->enc_cout[i], Ci = i == 0 ? 4 : a->enc_cin[i];
    CLSKD_CHECK_SHAPE(pow2(Co) && Co >= 2 && pow2(Ci) && Ci >= 4 && (i == 0 || Ci == a->enc_cout[i - 1]),
                      "stream_hop_mini: enc %d Ci=%d Co=%d", i, Ci, Co);
    CLSKD_CHECK_SHAPE(2 * Fi * Ci <= shop::WINSZ && Fo * Co <= 1024 && Ci <= 256 && 3 * Co + 2 <= 512 &&
                          plan_ok(Fo, Co, Ci, 1),
                      "stream_hop_mini: encoder %d too wide for the LDS budget", i);
    CLSKD_CHECK_ARG(a->enc_w[i] && a->enc_coef[i] && a->enc_alpha[i], "stream_hop_mini: enc %d", i);
  }
  CLSKD_CHECK_SHAPE((a->D4 << 6) == 256, "stream_hop_mini: D4=%d (six stride-2 encoders over 256 bins)", a->D4);
  for (int d = 0; d < 6; ++d) {
    const int F = a->D4 << d, Ca = a->dec_ca[d], Cb = a->dec_cb[d], Ci = Ca + Cb, Co = a->dec_co[d];
    CLSKD_CHECK_SHAPE(pow2(Co) && Co >= 2 && pow2(Ci) && Ci >= 4 && Ca >= 1 && Cb == a->enc_cout[5 - d] &&
                          Ca == (d == 0 ? a->enc_cout[5] : a->dec_co[d - 1]),
                      "stream_hop_mini: dec %d Ca=%d Cb=%d Co=%d", d, Ca, Cb, Co);
    CLSKD_CHECK_SHAPE(2 * F * Ci <= shop::WINSZ && 2 * F * Co <= 1024 && Ci <= 256 && 4 * Co + 2 <= 512 &&
                          plan_ok(F, Co, Ci, 2),
                      "stream_hop_mini: transposed conv %d too wide for the LDS budget", d);
    CLSKD_CHECK_ARG(a->dec_w[d][0] && a->dec_w[d][1] && (d == 5 || (a->dec_coef[d] && a->dec_alpha[d])),
                    "stream_hop_mini: dec %d weights", d);
  }
  CLSKD_CHECK_SHAPE(a->dec_co[5] == 2, "stream_hop_mini: the output layer emits (re, im), got %d", a->dec_co[5]);
  CLSKD_CHECK_SHAPE(2 * a->D4 * (a->enc_cout[5] / 2) <= shop::WINSZ && (a->D4 * a->enc_cout[5] / 2) % 4 == 0 &&
                        pow2(a->D4 * a->enc_cout[5] / 2) && 8 * a->H <= 512 && 2 * 4 * a->H <= 1024,
                    "stream_hop_mini: LSTM too wide for the LDS budget");
  for (int li = 0; li < 2; ++li)
    CLSKD_CHECK_ARG(a->lstm_w[li] && a->lstm_b[li] && a->lstm_whh[li], "stream_hop_mini: lstm %d", li);
  hipLaunchKernelGGL(stream_hop_mini_kernel, dim3((unsigned)a->B), dim3(shop::NT), 0, as_stream(stream), *a);
  CLSKD_LAUNCH_CHECK("stream_hop_mini");
  return CLSKD_OK;
}
