// One streaming hop of the DCCRN student (configuration C5) as ONE kernel launch.
//
// The hop-by-hop path (clskd/streaming.py, eager or hipGraph) issues ~70 small launches per
// 6.25 ms hop: ConvSTFT row, 6 encoder convs + BN/PReLU, 2 complex-LSTM steps, the projection,
// 12 polyphase decoder convs + BN/PReLU, mask 'E', the iSTFT row and the overlap-add — each a few
// hundred to a few thousand MACs per stream, so the hop is bound by launch and dependency
// latency (~10 us per node), not by arithmetic (3.8 MMAC per frame, DCCRN.py:149-240).
// Here one workgroup per stream walks the whole hop: every layer's current frame stays in LDS,
// the older frames the causal convolutions and the decoder look-ahead need live in per-stream
// rings in global memory (written by earlier hops, i.e. earlier launches: no cross-workgroup
// synchronisation at all), and the weights (3 MB of fp32 per hop, shared by every stream's
// workgroup through L2) go straight from L2 into registers in k-quad layout [K/4][N][4]: a lane
// owns one output channel and reads four k per 16-B load, a wavefront one contiguous 1 KB run,
// a batch of loads in flight per lane while the previous batch computes.  Each weight quad feeds
// up to 8 output rows and each activation quad (an LDS broadcast) 2 channels, accumulated as
// packed fp32 pairs (v_pk_fma_f32).  Layers whose output count leaves threads idle split K across threads and
// reduce through LDS, and both decoder parities run in the same pass, so every layer keeps all
// NT threads busy.  fp32 throughout, BatchNorm in eval mode (running statistics).
//
// Ring slots: frame f of a ring of depth D lives in slot ((f % D) + D) % D; rings start zeroed
// (the causal / centring zeros of the first frames).  Depths: spectrum 7 (mask of frame t-6),
// encoder output i: 7 - i (decoder 5 - i reads frames t-6+i, t-5+i), decoder input 2, decoder
// output d: 2, iSTFT frames 4 (the 400-sample window spans 4 hops).
#include "common.h"

namespace clskd {
#ifdef CLSKD_EXPERIMENTS
// phase timestamps of stream 0 (thread 0, after each phase's barrier): diagnostic only
__device__ uint64_t g_hop_marks[40];
#define CMARK(i)                                                                          \
  do {                                                                                    \
    if ((i) >= 0 && blockIdx.x == 0 && threadIdx.x == 0) g_hop_marks[i] = wall_clock64(); \
  } while (0)
#else
#define CMARK(i) \
  do {           \
  } while (0)
#endif
}  // namespace clskd

#include "stream_hop_common.h"

namespace clskd {
#define HOP_MARK(i) CMARK(i)

__global__ __launch_bounds__(shop::NT) void stream_hop_kernel(const clskd_stream_hop_args a) {
  using namespace shop;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int t = a.t;
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
  __shared__ float cv[2][2][64], act[2][2][4 * 64];
  __shared__ __attribute__((aligned(16))) float rin[2][64];
  __shared__ __attribute__((aligned(16))) float est[LDEST];
  __shared__ __attribute__((aligned(16))) float frame[WIN];
  __shared__ __attribute__((aligned(16))) float red[RED];
  __shared__ __attribute__((aligned(16))) float prm[512];
  __shared__ __attribute__((aligned(16))) float whh[8 * 32 * 36];  // W_hh [2*4H][H + 4], H <= 32

  HOP_MARK(0);
#ifdef CLSKD_EXPERIMENTS
  if (b == 0 && tid == 0) {  // shader-clock rate and one dependent global round trip
    const uint64_t w0 = wall_clock64();
    g_hop_marks[38] = clock64();
    const float v = ldg(a.enc_w[3] + 64 * (t % 16));
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t c0 = clock64();
    g_hop_marks[30] = c0 - (uint64_t)(v == 12345.f);  // (v consumed: the load completes before c0)
    g_hop_marks[31] = w0;
  }
#endif
  for (int i = tid; i < 256; i += NT) win[ZOFF + i] = 0.f;
  const float* zr = win + ZOFF;  // zero row (LDS)
  // ---- input window: shift by one hop, append the new samples (tools_for_model.py:53-67)
  float* gxw = st + a.off_xwin;
  auto stage_x = [&]() {
    for (int i = tid; i < WIN; i += NT)
      xw[i] = i < WIN - HOP ? gxw[i + HOP] : (a.live ? a.x_in[(int64_t)b * HOP + i - (WIN - HOP)] : 0.f);
  };

  float* cur = curA;
  float* nxt = curB;
  if (a.live) {
    // ---- ConvSTFT row of the newest window -> spectrum ring
    gemv(a.stft_w, nullptr, L(xw), 0, 1, WIN / 4, NBIN, L(spec), 0, L(red), L(zr), stage_x);
    __syncthreads();
    HOP_MARK(1);
    // ---- encoder (DCCRN.py:171-176): window [t-1, t], taps (kf - 2, kt), stride 2 in F.
    //      The ring writes of the previous phase's output are issued in the next phase's staging,
    //      behind its first weight loads: gfx950's vmcnt counts stores, so a load issued after a
    //      store would wait for that store's acknowledgement too.
    for (int i = 0; i < 6; ++i) {
      const int Fi = 256 >> i, Fo = Fi / 2, Co = a.enc_cout[i];
      const int Ci = i == 0 ? 4 : a.enc_cin[i];  // encoder 0: (re, im) padded to a quad
      // stage [2][Fi][Ci]: slot 1 = this frame (spectrum / previous layer in LDS), slot 0 = t-1
      auto stage = [&]() {
        if (i == 0) {
          for (int j = tid; j < WIN; j += NT) gxw[j] = xw[j];  // (every read of gxw is behind gemv's barrier)
          float* sring = st + a.off_spec;
          for (int j = tid; j < NBIN; j += NT) sring[ring(t, 7) * NBIN + j] = spec[j];
          const float* sp = st + a.off_spec + ring(t - 1, 7) * NBIN;
          for (int q = tid; q < 4 * Fi; q += NT) {
            const int f = q >> 2, ri = q & 3;
            win[q] = ri < 2 ? sp[(ri ? 258 : 1) + f] : 0.f;
            win[4 * Fi + q] = ri < 2 ? spec[(ri ? 258 : 1) + f] : 0.f;
          }
        } else {
          const int D = 7 - (i - 1);
          float* ep = st + a.off_enc[i - 1];
          const float* rp = ep + (int64_t)ring(t - 1, D) * Fi * Ci;
          float* er = ep + (int64_t)ring(t, D) * Fi * Ci;  // encoder i-1's frame t (its output Fi x Ci)
          for (int q = tid; q < Fi * Ci; q += NT) {
            win[q] = rp[q];
            win[Fi * Ci + q] = cur[q];
            er[q] = cur[q];
          }
        }
      };
      const Geo g{Fi, Ci, 31 - __builtin_clz(Ci / 4), 2, 0};
      conv_layer(L(win), g, 1, 10 * Ci / 4, 0, Fo, Co, a.enc_w[i], nullptr, a.enc_b[i], nullptr, a.enc_coef[i],
                 a.enc_alpha[i], L(nxt), 1, L(red), L(prm), false, i == 0 ? 32 : i == 4 ? 34 : -1, stage);
      __syncthreads();
      HOP_MARK(2 + i);
      float* tmp = cur;
      cur = nxt;
      nxt = tmp;
    }
    // cur = encoder 5 output [D4][C6] of frame t
    // ---- complex LSTMs (DCCRN.py:178-199), (h, c) carried across hops
    lstm_hop(LstmLds{L(win), L(&gx[0][0]), L(&hv[0][0][0]), L(&cv[0][0][0]), L(&act[0][0][0]), L(whh),
                     L(&rin[0][0]), L(red), L(zr), L(cur)},
             64, st + a.off_enc[5] + (int64_t)ring(t, 2) * D4 * C6, a.lstm_w, a.lstm_b, a.lstm_whh,
             st + a.off_h, st + a.off_c, H, D4, C6);
    // projection (NavieComplexLSTM r_trans / i_trans): dec_in[f][half*Ch + c], n = c*D4 + f
    float* pj = &act[0][0][0];  // [2][Ch*D4] (the gate scratch is free now)
    for (int half = 0; half < 2; ++half) {
      gemv(a.proj_w[half], a.proj_b[half], L(rin[half]), 0, 1, H / 4, Ch * D4, L(pj + half * Ch * D4), 0, L(red),
           L(zr), []() {});
      __syncthreads();
    }
    for (int q = tid; q < 2 * Ch * D4; q += NT) {
      const int ld4 = lg2(D4), lcd = lg2(Ch) + ld4;
      const int half = q >> lcd, n = q & ((1 << lcd) - 1);
      decin[(n & (D4 - 1)) * C6 + half * Ch + (n >> ld4)] = pj[q];
    }
    __syncthreads();
    HOP_MARK(10);
  } else {
    // drain hop: no new frame; encoder outputs and the decoder input of frame t are zeros
    stage_x();
    __syncthreads();
    for (int i = tid; i < WIN; i += NT) gxw[i] = xw[i];
    for (int i = 0; i < 6; ++i) {
      const int Fo = 128 >> i, Co = a.enc_cout[i];
      float* er = st + a.off_enc[i] + (int64_t)ring(t, 7 - i) * Fo * Co;
      for (int q = tid; q < Fo * Co; q += NT) er[q] = 0.f;
    }
    for (int q = tid; q < D4 * C6; q += NT) {
      cur[q] = 0.f;
      decin[q] = 0.f;
    }
    __syncthreads();
  }

  // ---- decoder (DCCRN.py:201-206): layer d emits frame t-1-d from its input's frames
  //      [t-1-d, t-d] and encoder 5-d's frames [t-1-d, t-d]; both parities in one pass
  const float* in_cur = decin;  // frame t-d of this layer's input
  for (int d = 0; d < 6; ++d) {
    const int F = D4 << d, Ca = a.dec_ca[d], Cb = a.dec_cb[d], Ci = Ca + Cb, Co = a.dec_co[d];
    const int ie = 5 - d, De = 7 - ie;
    const int out_frame = t - 1 - d;
    const bool dead = a.zero_from >= 0 && out_frame >= a.zero_from;
    const float* in_old = d == 0 ? st + a.off_decin + ring(t - 1, 2) * D4 * C6
                                 : st + a.off_dout[d - 1] + (int64_t)ring(t - 1 - d, 2) * F * Ca;
    const float* sk_old = st + a.off_enc[ie] + (int64_t)ring(t - 1 - d, De) * F * Cb;
    const float* sk_new = d == 0 ? cur : st + a.off_enc[ie] + (int64_t)ring(t - d, De) * F * Cb;
    const bool last = d == 5;
    // _DEC_TAPS (model.py): parity 0 -> dF (1, 0, -1), parity 1 -> dF (1, 0); K order per tap
    // (kt = 0, 1) with window slot 1 - kt
    const Geo g{F, Ci, 31 - __builtin_clz(Ci / 4), 1, 1};
    conv_layer(L(win), g, 2, 6 * Ci / 4, 4 * Ci / 4, F, Co, a.dec_w[d][0], a.dec_w[d][1], a.dec_b[d][0],
               a.dec_b[d][1], last ? nullptr : a.dec_coef[d], last ? nullptr : a.dec_alpha[d], L(nxt), 2, L(red),
               L(prm), dead, d == 1 ? 36 : -1, [&]() {
                 // the previous phase's output -> its ring (behind this layer's first weight loads)
                 if (d == 0) {
                   float* dr = st + a.off_decin + ring(t, 2) * D4 * C6;
                   for (int q = tid; q < D4 * C6; q += NT) dr[q] = decin[q];
                 } else {  // decoder d-1's frame t-d: [2 F_{d-1} = F][Co_{d-1} = Ca]
                   float* orr = st + a.off_dout[d - 1] + (int64_t)ring(t - d, 2) * F * Ca;
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
    HOP_MARK(11 + d);
  }
  // in_cur = mask of frame t-6: [256][2] (re, im)
  // ---- mask 'E' (DCCRN.py:207-226) on the spectrum of frame t-6 (staged while the first iSTFT
  //      weight batches load), ConviSTFT row, overlap-add
  const float* s6 = st + a.off_spec + ring(t - 6, 7) * NBIN;
  HOP_MARK(17);
  gemv(a.istft_w, nullptr, L(est), 0, 1, LDEST / 4, WIN, L(frame), 0, L(red), L(zr), [&]() {
    for (int f = tid; f < 257; f += NT) {
      const float re = s6[f], im = s6[257 + f];
      const float mags = sqrtf(re * re + im * im + 1e-8f);
      const float phase = atan2f(im, re);
      float mr = 0.f, mi = 0.f;
      if (f > 0) {
        mr = in_cur[(f - 1) * 2];
        mi = in_cur[(f - 1) * 2 + 1];
      }
      const float mm = sqrtf(mr * mr + mi * mi);
      const float rp = mr / (mm + 1e-8f);
      const float ip = mi / (mm + 1e-8f);
      const float mphase = atan2f(ip, rp);
      const float em = tanhf(mm) * mags;
      const float ep = phase + mphase;
      est[f] = em * cosf(ep);
      est[257 + f] = em * sinf(ep);
    }
    if (tid < 2) est[514 + tid] = 0.f;
  });
  __syncthreads();
  HOP_MARK(18);
  float* fr = st + a.off_frames;
  for (int i = tid; i < WIN; i += NT) fr[ring(t, 4) * WIN + i] = frame[i];
  // output samples of this hop: p = n + 300 over the frames t-3 .. t (k = 0 .. 3)
  for (int n = tid; n < HOP; n += NT) {
    const int p = n + 300;
    float acc = 0.f, coff = 0.f;
    for (int k = 0; k < 4; ++k) {
      const int o = p - k * HOP;
      if (o < 0 || o >= WIN) continue;
      const float v = k == 3 ? frame[o] : fr[ring(t - 3 + k, 4) * WIN + o];
      acc += v;
      const float w = a.window[o];
      coff += w * w;
    }
    float v = acc / (coff + 1e-8f);
    v = fminf(fmaxf(v, -1.f), 1.f);
    a.wav_out[(int64_t)b * HOP + n] = v;
  }
  HOP_MARK(19);
#ifdef CLSKD_EXPERIMENTS
  if (b == 0 && tid == 0) g_hop_marks[39] = clock64();
#endif
}

}  // namespace clskd

using namespace clskd;

extern "C" int clskd_stream_hop(const clskd_stream_hop_args* a, void* stream) {
  CLSKD_CHECK_ARG(a && a->state && a->wav_out && a->stft_w && a->istft_w && a->window,
                  "stream_hop: null argument");
  CLSKD_CHECK_ARG(!a->live || a->x_in, "stream_hop: live hop without input");
  CLSKD_CHECK_SHAPE(a->B >= 1 && a->t >= 0, "stream_hop: B=%d t=%d", a->B, a->t);
  auto pow2 = [](int v) { return v >= 1 && (v & (v - 1)) == 0; };
  CLSKD_CHECK_SHAPE(a->H >= 4 && pow2(a->H) && 16 * a->H <= shop::NT && a->D4 >= 1 &&
                        pow2(a->D4) && a->D4 * a->enc_cout[5] <= 256 && a->enc_cout[5] % 2 == 0,
                    "stream_hop: H=%d D4=%d outside the built LDS budget", a->H, a->D4);
  CLSKD_CHECK_SHAPE(a->enc_cin[0] == 2, "stream_hop: encoder 0 takes (re, im), got %d", a->enc_cin[0]);
  // conv_layer's thread plans: R = 8 rows (4 where Fo == 4), CQ = 2 channels where Co >= 16 (or
  // Fo == 4); the plan's (rows / R) * (Co / CQ) per parity must fit the block.
  auto plan_ok = [&](int Fo, int Co, int Ci, int np) {
    const int R = Fo >= 8 ? 8 : 4, CQ = (Fo < 8 || Co >= 16) ? 2 : 1;
    return pow2(Fo) && Fo >= 4 && (Fo >= 8 || (Co >= 16 && Ci >= 16)) && np * (Fo / R) * (Co / CQ) <= shop::NT &&
           Co % CQ == 0;
  };
  for (int i = 0; i < 6; ++i) {
    const int Fi = 256 >> i, Fo = Fi / 2, Co = a->enc_cout[i], Ci = i == 0 ? 4 : a->enc_cin[i];
    CLSKD_CHECK_SHAPE(pow2(Co) && pow2(Ci) && Ci >= 4 && (i == 0 || Ci == a->enc_cout[i - 1]),
                      "stream_hop: enc %d Ci=%d Co=%d", i, Ci, Co);
    CLSKD_CHECK_SHAPE(2 * Fi * Ci <= shop::WINSZ && Fo * Co <= 1024 && Ci <= 256 && plan_ok(Fo, Co, Ci, 1),
                      "stream_hop: encoder %d too wide for the LDS budget", i);
    CLSKD_CHECK_ARG(a->enc_w[i] && a->enc_b[i] && a->enc_coef[i] && a->enc_alpha[i], "stream_hop: enc %d", i);
  }
  for (int d = 0; d < 6; ++d) {
    const int F = a->D4 << d, Ci = a->dec_ca[d] + a->dec_cb[d], Co = a->dec_co[d];
    CLSKD_CHECK_SHAPE(pow2(Co) && pow2(Ci) && Ci >= 4, "stream_hop: dec %d Ci=%d Co=%d", d, Ci, Co);
    CLSKD_CHECK_SHAPE(2 * F * Ci <= shop::WINSZ && 2 * F * Co <= 1024 && Ci <= 256 && plan_ok(F, Co, Ci, 2),
                      "stream_hop: decoder %d too wide for the LDS budget", d);
    CLSKD_CHECK_ARG(a->dec_w[d][0] && a->dec_w[d][1], "stream_hop: dec %d weights", d);
  }
  CLSKD_CHECK_SHAPE(2 * a->D4 * (a->enc_cout[5] / 2) <= shop::WINSZ && (a->D4 * a->enc_cout[5] / 2) % 4 == 0 &&
                        8 * a->H <= 512 && 2 * 4 * a->H <= 1024,
                    "stream_hop: LSTM too wide for the LDS budget");
  hipLaunchKernelGGL(stream_hop_kernel, dim3((unsigned)a->B), dim3(shop::NT), 0, as_stream(stream), *a);
  CLSKD_LAUNCH_CHECK("stream_hop");
  return CLSKD_OK;
}

extern "C" int clskd_stream_hop_marks(int64_t* out, int32_t n) {
#ifdef CLSKD_EXPERIMENTS
  CLSKD_CHECK_ARG(out && n >= 1 && n <= 40, "stream_hop_marks: bad output");
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hop_marks), sizeof(int64_t) * n) != hipSuccess) {
    set_error("stream_hop_marks: copy failed");
    return CLSKD_E_HIP;
  }
  return CLSKD_OK;
#else
  (void)out;
  (void)n;
  set_error("stream_hop_marks: phase marks exist only in a -DCLSKD_EXPERIMENTS build");
  return CLSKD_E_ARG;
#endif
}
