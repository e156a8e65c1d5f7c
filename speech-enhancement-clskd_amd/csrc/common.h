// Shared device/host helpers for libclskd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/clskd.h"

namespace clskd {

// ---- host-side error plumbing (thread-local message; no exceptions across the C ABI) ----------
void set_error(const char* fmt, ...);
// Instance name of the kernel the calling thread's last conv launch ran ("base<arg,...>", the
// template arguments rocprof shows); read back through clskd_conv_last_kernel().
void note_kernel(const char* fmt, ...);
// Host function of that kernel (clskd_conv_last_kernel_fn: the executor's per-kernel timing key).
void note_kernel_fn(const void* fn);
// Dispatch knobs (capi.cpp): env read once at first use, changed only by clskd_set_knob.
// The one list of knobs, X(name, default, product): KNOB_<name> here and the registry entry
// "CLSKD_<name>" in capi.cpp both come from it.  Product knobs are parity-tested dispatch routes
// (tests/test_gpu_parity.py); every other knob is an A/B or timing experiment: a product build
// holds it at its default (the environment is not read for it and clskd_set_knob refuses another
// value).
#define CLSKD_KNOBS(X) \
  X(G8, 1, false) X(G8_GRID, 0, true) X(HALO_GRID, 0, false) X(LSTM_NKS, 4, false)             \
  X(LSTM_NKS32, 1, true) X(WGRAD_WG, 4096, false) X(NO_HALO, 0, false) X(BF16_WAVES, 8, false) \
  X(BF16_STAGES, 3, false) X(BF16_TILE, 0, false) X(NO_POINTWISE, 0, false)                    \
  X(ABF_MOMENT_DIV, 1, false) X(F32_WAVES, 4, false) X(EXEC_GATE, 0, false)                    \
  X(NO_HALO32, 0, true) X(HALO32_SPLIT, 0, true) X(HALO32_MIN_N, 32, true)                     \
  X(G8_KORDER, 1, false) X(G8_PP, 0, false) X(F32_SPLIT, 0, true) X(LSTM_PRIO, 0, true)        \
  X(SPLIT_BK, 0, true) X(HALOW, 0, false) X(SPLIT_GRID, 0, true) X(G8_TA, 1, true)             \
  X(G8_SK, 1, true) X(SPLIT_PD, 1, true) X(SPLIT_OCC, 1, true) X(WGRAD_DEPTH, 0, true)         \
  X(LSTM_BWD_WAVE, 1, true) X(SPLIT_NS2, 1, true) X(BN_PFOLD, 1, true) X(LSTM_PRE, 1, true)    \
  X(ABF_BWD_BLOCKS, 2048, false) X(WGRAD_XCD, 1, true) X(LSTM_BWD_PIN, 1, true)                \
  X(HALO_SPLIT, 1, true) X(HALO_SPLIT_GRID, 0, true)                                           \
  /* timing-only experiment modes (wrong results): -DCLSKD_EXPERIMENTS builds only */          \
  X(LSTM128_TDIV, 0, false) X(LSTM32_TDIV, 0, false) X(BF16_DEBUG_MODE, 0, false)              \
  X(SKIP, 0, false) X(H32_DEBUG_MODE, 0, false)
enum KnobId {
#define X(name, dflt, product) KNOB_##name,
  CLSKD_KNOBS(X)
#undef X
  KNOB_COUNT
};
int knob(KnobId k);
// In-place level-2 fold of a [nblk][E] fp64 partial table before a one-workgroup-per-channel
// finalize (norm.hip): returns the row count the finalize then reads (nblk when not folded).
// `bit` = 1 backward finalizes, 2 forward (CLSKD_BN_PFOLD mask).
int fold_partials(double* part, int nblk, int E, int bit, hipStream_t st);
// The PReLU slope gradient of the BatchNorm and ComplexBatchNorm backwards (norm_bwd.hip):
// dalpha[h] (+)= sum of alpha_part over the channels of part h of `halves` equal parts, ascending.
void bn_bwd_alpha(const double* alpha_part, int C, int halves, float* dalpha, int accumulate,
                  hipStream_t st);
// CLSKD_OK, or CLSKD_E_ARG (with the error message set) when `value` selects a timing-only mode
// in a product build.
int experiment_guard(const char* what, int value);
// Timing-only "what if this kernel family were free" switch (CLSKD_SKIP bit mask, experiments
// build only; always false in the product library): the entry point returns without launching.
enum SkipBit {
  SKIP_BN_FINALIZE = 1, SKIP_BN_APPLY = 2, SKIP_CONV_F32 = 4, SKIP_LSTM = 8, SKIP_ABF = 16,
  SKIP_GRAM = 32, SKIP_CONV_LOWP = 64, SKIP_CONV_DIRECT = 128, SKIP_LSTM_PRE = 256, SKIP_LSTM_BWD = 512
};
bool skip_kernel(int bit);
template <typename T> inline const char* type_name();
template <> inline const char* type_name<float>() { return "float"; }
template <> inline const char* type_name<__bf16>() { return "bf16"; }
template <> inline const char* type_name<_Float16>() { return "f16"; }
// storage-type code of a 16-bit type (clskd_compute)
template <typename T> constexpr int lowp_code() { return sizeof(T) == 4 ? CLSKD_F32 : CLSKD_BF16; }
template <> constexpr int lowp_code<_Float16>() { return CLSKD_F16; }
inline bool is_lowp(int dt) { return dt == CLSKD_BF16 || dt == CLSKD_F16; }

#define CLSKD_CHECK_ARG(cond, ...)                 \
  do {                                             \
    if (!(cond)) {                                 \
      ::clskd::set_error(__VA_ARGS__);             \
      return CLSKD_E_ARG;                          \
    }                                              \
  } while (0)

#define CLSKD_CHECK_SHAPE(cond, ...)               \
  do {                                             \
    if (!(cond)) {                                 \
      ::clskd::set_error(__VA_ARGS__);             \
      return CLSKD_E_SHAPE;                        \
    }                                              \
  } while (0)

#define CLSKD_LAUNCH_CHECK(name)                                                  \
  do {                                                                            \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess) {                                                       \
      ::clskd::set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
      return CLSKD_E_HIP;                                                         \
    }                                                                             \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// blocks of a 256-thread grid-stride pass over n items: at least one, at most `cap`
inline unsigned grid_for(int64_t n, int64_t cap = 8192) {
  const int64_t g = cdiv(n, 256);
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// compute units of device 0, read once (capi.cpp); 256 when there is no device to ask
int device_cu_count();

// ---- device helpers ---------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 4 channels of fp32 / bf16 storage <-> f32x4 (8- or 16-B accesses)
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// hi / lo bf16 split of 4 fp32 values (RNE both): the operands of the 3 x bf16 split products
__device__ __forceinline__ void split4(const f32x4 v, s16x4& hi, s16x4& lo) {
  bf16x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = (__bf16)v[i];
    l[i] = (__bf16)(v[i] - (float)h[i]);
  }
  hi = __builtin_bit_cast(s16x4, h);
  lo = __builtin_bit_cast(s16x4, l);
}

// One 1-KiB LDS-DMA wave instruction: lane l copies 16 B from gsrc to lds_base + 16*l.  Inline
// asm (cdna_hip_programming.md §5.7): hipcc neither tracks nor waits for it, so a kernel's counted
// vmcnt waits are the only synchronisation.  M0 is set and restored inside.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_base)
      : "memory");
}

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
template <>
__device__ __forceinline__ f32x4 load4<__bf16>(const __bf16* p) {
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <>
__device__ __forceinline__ f32x4 load4<_Float16>(const _Float16* p) {
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <typename T>
__device__ __forceinline__ void store4(T* p, f32x4 v);
template <>
__device__ __forceinline__ void store4<float>(float* p, f32x4 v) {
  *reinterpret_cast<f32x4*>(p) = v;
}
template <>
__device__ __forceinline__ void store4<__bf16>(__bf16* p, f32x4 v) {
  bf16x4 o;
  o[0] = (__bf16)v[0];
  o[1] = (__bf16)v[1];
  o[2] = (__bf16)v[2];
  o[3] = (__bf16)v[3];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// one v_mfma_f32_32x32x16 on 16-bit operands held as any 16-byte vector (8 lanes of bf16 or
// IEEE half bits): InT selects the bf16 or the f16 instruction (same rate on gfx950)
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
template <typename InT, typename V>
__device__ __forceinline__ f32x16 mfma16(const V& a, const V& b, const f32x16& c) {
  static_assert(sizeof(V) == 16, "8 x 16-bit operand lanes");
  if constexpr (__is_same(InT, _Float16))
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a),
                                                  __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// XCD-aware tile order: the hardware places workgroup i on XCD i % 8.  Give every XCD one
// contiguous run of M-tiles (a bijection on [0, nb)), so neighbouring tiles — which read
// overlapping input rows through the conv taps — share that XCD's L2 instead of each of the
// eight L2s fetching the same rows.
__device__ __forceinline__ int xcd_tile(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7, x = bid & 7, j = bid >> 3;
  return x * q + (x < r ? x : r) + j;
}

// ---- clskd_conv_desc's output map, and small helpers more than one conv kernel family uses ----
// element offset of output row (b, fo, to): of_mul / of_add interleave the polyphase decoder rows
__host__ __device__ __forceinline__ int64_t conv_out_row(const clskd_conv_desc& d, int64_t b, int fo, int to) {
  return b * d.oB + (int64_t)(fo * d.of_mul + d.of_add) * d.oF + (int64_t)to * d.oT;
}
// element offset of output column n (split column map: n = hi * nlo + lo)
__host__ __device__ __forceinline__ int64_t conv_col_off(const clskd_conv_desc& d, int n) {
  return (int64_t)(n / d.nlo) * d.oNhi + (int64_t)(n % d.nlo) * d.oNlo;
}
// row inside a 32x32 MFMA accumulator of element r (0..15) held by lane half h
__host__ __device__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// select the per-segment value without runtime-indexed arrays (which would go to scratch): two
// levels of value selects (v_cndmask); an if-else chain compiles to exec-mask branches
template <typename T>
__device__ __forceinline__ T sel4(int s, T a0, T a1, T a2, T a3) {
  const T lo = (s & 1) ? a1 : a0;
  const T hi = (s & 1) ? a3 : a2;
  return (s & 2) ? hi : lo;
}

// the if-else chain form: conv_bf16.hip and conv_direct.hip lose occupancy with the select tree
template <typename T>
__device__ __forceinline__ T sel4_chain(int s, T a0, T a1, T a2, T a3) {
  return s == 0 ? a0 : (s == 1 ? a1 : (s == 2 ? a2 : a3));
}

template <typename OutT>
__device__ __forceinline__ void store_out(OutT* p, float v) { *p = (OutT)v; }

// vmcnt takes immediates only: wait until at most n of this wave's VMEM ops are outstanding
template <int MAXN>
__device__ __forceinline__ void wait_vm(int n) {
  if constexpr (MAXN <= 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if (n >= MAXN) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MAXN) : "memory");
    else wait_vm<MAXN - 1>(n);
  }
}

// raw workgroup barrier that leaves LDS-DMA in flight: this wave's LDS reads/writes retired
// first (lgkmcnt), then s_barrier; the compiler may not move memory operations across it
__device__ __forceinline__ void raw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// LSTM gate nonlinearities on v_exp_f32 / v_rcp_f32 (~1 ulp each; the recurrence's fp32 rounding,
// not these, dominates its error against the oracle).  One definition for the offline recurrence
// (lstm.hip) and the fused streaming hops, so a stream of hops reproduces the offline sequence.
__device__ __forceinline__ float sigm_fast(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f));
}
__device__ __forceinline__ float tanh_fast(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * 2.8853900817779268f));
}
// the tanh of the g gate, on the sigmoid's instructions: 2 sigmoid(2x) - 1
__device__ __forceinline__ float tanh_gate(float x) { return fmaf(2.f, sigm_fast(2.f * x), -1.f); }

// scale/shift (and batch mean/var, running stats) of one channel from its totals.
__device__ __forceinline__ void bn_channel_coeffs(int c, double S, double Q, int64_t rows,
                                                  const float* gamma, const float* beta, float eps,
                                                  float* running_mean, float* running_var,
                                                  float momentum, int n_updates, float* scale,
                                                  float* shift, float* mean_out, float* var_out) {
  const double n = (double)rows;
  const double mean = S / n;
  double var = Q / n - mean * mean;
  if (var < 0) var = 0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[c] : 1.f;
  const float bb = beta ? beta[c] : 0.f;
  const float sc = invstd * g;
  scale[c] = sc;
  shift[c] = bb - (float)mean * sc;
  if (mean_out) mean_out[c] = (float)mean;
  if (var_out) var_out[c] = (float)var;
  if (running_mean && running_var) {
    const float unb = (float)(rows > 1 ? var * n / (n - 1.0) : var);
    float rm = running_mean[c], rv = running_var[c];
    for (int u = 0; u < n_updates; ++u) {
      rm = (1.f - momentum) * rm + momentum * (float)mean;
      rv = (1.f - momentum) * rv + momentum * unb;
    }
    running_mean[c] = rm;
    running_var[c] = rv;
  }
}


// ATen nearest_idx (UpSample.h) for F.interpolate(mode="nearest"): source index of dst.
__device__ __forceinline__ int nearest_src(int dst, int in_size, int out_size) {
  // ATen nearest_idx (UpSample.h): identity / >>1 fast paths, else floorf(dst*scale), scale in f32
  if (out_size == in_size) return dst;
  if (out_size == 2 * in_size) return dst >> 1;
  const float scale = (float)in_size / (float)out_size;
  const int s = (int)floorf((float)dst * scale);
  return s < in_size - 1 ? s : in_size - 1;
}

// masking mode 'E' (norm.hip mask_e_kernel, norm_bwd.hip mask_e_bwd_kernel): MASK_TT frames per
// block; the mask columns [256][2 * MASK_TT] staged in LDS with a padded row (MASK_LD floats: the
// bins of one wave's float2 reads fall on distinct banks)
constexpr int MASK_TT = 16;
constexpr int MASK_LD = 2 * MASK_TT + 2;
// ml[fm][r] = mcol[fm * Tm * 2 + r] for r < 2 * nt (mcol: the block's first column of bin 0)
__device__ __forceinline__ void mask_tile_load(const float* __restrict__ mcol, int Tm, int nt,
                                               float* ml) {
  for (int i = threadIdx.x; i < 256 * 2 * MASK_TT; i += blockDim.x) {
    const int fm = i / (2 * MASK_TT), r = i - fm * 2 * MASK_TT;
    if (r < 2 * nt) ml[fm * MASK_LD + r] = mcol[(int64_t)fm * Tm * 2 + r];
  }
}
// the backward twin: dcol[fm * Tm * 2 + r] = ml[fm][r] for r < 2 * nt (the mask gradient of the
// block's frames, in the same runs), and for the block with first = true the columns of the
// utterance's mask (dutt: its [256][Tm][2]) that no frame reads — tm = 0 and T < tm < Tm — as zero.
// For blocks of 256 threads (the mask backward kernels' launch bounds).
__device__ __forceinline__ void mask_tile_store(float* __restrict__ dcol, float* __restrict__ dutt,
                                                int Tm, int T, int nt, bool first,
                                                const float* ml) {
  for (int i = threadIdx.x; i < 256 * 2 * MASK_TT; i += 256) {
    const int fm = i / (2 * MASK_TT), r = i - fm * 2 * MASK_TT;
    if (r < 2 * nt) dcol[(int64_t)fm * Tm * 2 + r] = ml[fm * MASK_LD + r];
  }
  if (first) {
    const int nz = Tm - T;
    for (int i = threadIdx.x; i < 256 * nz; i += 256) {
      const int fm = i / nz, j = i - fm * nz;
      const int tm = j == 0 ? 0 : T + j;
      float* dp = dutt + ((int64_t)fm * Tm + tm) * 2;
      dp[0] = 0.f;
      dp[1] = 0.f;
    }
  }
}

}  // namespace clskd
