// The stages the frame kernels share (impair.hip, synth.hip, waveform.hip, receiver.hip, spectrogram.hip, cyclic.hip): one
// workgroup of FR_THREADS per frame (or per frame and band), the frame in LDS.  Everything here takes plain values and pointers
// and knows nothing of the kernel that calls it; what differs in substance between two kernels stays in their files.
//   every file    FR_* constants, frame_fits, frame_vec4, is_finite, launch_frames, red_sum
//   transmitters  frame_key, draw_class_snr, rotate, noise4, scan_exclusive, frame_scale + store_frame (the generators' tail),
//                 synth_lists_ok, pack_synth_lists
//   channelizers  f32x16, acc_row, frame_floats, window_start, stage_frame, channel_step, overlap_add, power, scale_shift,
//                 image_value, fft_size_ok
//   symbol stages load_sample, store_sample
#pragma once
#include <math.h>

#include "common.h"

constexpr int FR_THREADS = 256;
constexpr int FR_WAVES = FR_THREADS / IQ_WAVE;
constexpr size_t FR_MAX_FRAME_BYTES = 64 * 1024;   // one frame (len * 8 bytes) stays in LDS
constexpr uint32_t FR_PARAM_CTR = 0xFFFFFFFFu;     // the frame's parameters: never a symbol, sample-pair or noise group (len * 8 <= 64 KB)
constexpr float FR_TWO_PI = 6.28318530717958647692f;
constexpr float FR_RSQRT2 = 0.70710678118654752440f;
constexpr int FR_MIN_FFT = 32, FR_MAX_FFT = 256, FR_TILE = 32;   // the channelizers' MFMA tile edge and table sizes

// ---- host: refusals and the launch
inline bool is_finite(float v) { return fabsf(v) < INFINITY; }
inline bool frame_fits(int len) { return (size_t)len * 8 <= FR_MAX_FRAME_BYTES; }
inline bool fft_size_ok(int n_fft) { return n_fft >= FR_MIN_FFT && n_fft <= FR_MAX_FFT && n_fft % FR_TILE == 0; }
// every frame of `p` starts 16-byte aligned and is a whole number of 16-byte groups: float4 loads / stores
inline int frame_vec4(const void* p, int len) { return (len % 2 == 0 && ((uintptr_t)p & 15) == 0) ? 1 : 0; }

template <typename Args>
inline void launch_frames(void (*kernel)(Args), dim3 grid, size_t lds, hipStream_t st, const Args& a) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kernel<<<grid, FR_THREADS, lds, st>>>(a);
}

// The class / SNR lists of iq_synth_t and iq_waveform_t: true when a generator may read them (every failure is an IQ_ERR_ARG).
// Only the entries a kernel could use are looked at; a list longer than the kernel's arrays is refused as unsupported later.
inline bool synth_lists_ok(const iq_synth_class_t* classes, int n_classes, const float* snrs_db, int n_snrs, const float* points,
                           int balanced) {
  if (!classes || n_classes <= 0 || n_snrs < 0 || (n_snrs > 0 && !snrs_db)) return false;
  if (balanced & ~1) return false;
  const int nc = n_classes < IQ_SYNTH_MAX_CLASSES ? n_classes : IQ_SYNTH_MAX_CLASSES;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = classes[i];
    if (c.kind < 0 || c.kind > 2) return false;
    if (c.kind == 0 && (c.count <= 0 || c.offset < 0 || !points)) return false;
  }
  const int ns = n_snrs < IQ_SYNTH_MAX_SNRS ? n_snrs : IQ_SYNTH_MAX_SNRS;
  for (int i = 0; i < ns; ++i)
    if (!is_finite(snrs_db[i])) return false;
  return true;
}
// The lists as kernel arguments, padded with a class that reads no table and with 0 dB.
inline void pack_synth_lists(iq_synth_class_t* classes_out, float* snrs_out, const iq_synth_class_t* classes, int n_classes,
                             const float* snrs_db, int n_snrs) {
  for (int i = 0; i < IQ_SYNTH_MAX_CLASSES; ++i) classes_out[i] = i < n_classes ? classes[i] : iq_synth_class_t{1, 0, 0};
  for (int i = 0; i < IQ_SYNTH_MAX_SNRS; ++i) snrs_out[i] = i < n_snrs ? snrs_db[i] : 0.f;
}

// ---- transmitters
// frame = frame_base + block; Philox key (k0, k1) = (seed lo, seed hi ^ frame hi), counter word 1 = frame lo
struct FrameKey {
  uint64_t frame;
  uint32_t k0, k1, flo;
};
__device__ __forceinline__ FrameKey frame_key(uint64_t seed, uint64_t frame_base, uint32_t block) {
  const uint64_t frame = frame_base + (uint64_t)block;
  return FrameKey{frame, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(frame >> 32), (uint32_t)frame};
}

// balanced: class frame % K, SNR index (frame / K) % n_snrs; otherwise words 1 and 2 of the parameter draw.  si = 0 without noise.
__device__ __forceinline__ void draw_class_snr(uint64_t frame, u32x4 par, int balanced, int n_classes, int n_snrs, bool noise,
                                               int& cls, int& si) {
  si = 0;
  if (balanced) {
    cls = (int)(frame % (uint64_t)n_classes);
    if (noise) si = (int)((frame / (uint64_t)n_classes) % (uint64_t)n_snrs);
  } else {
    cls = (int)__umulhi(par[1], (uint32_t)n_classes);
    if (noise) si = (int)__umulhi(par[2], (uint32_t)n_snrs);
  }
}

// v * (c0 + i s0), every rounding spelled out (one product rounded, the other fused): the same bits wherever it is compiled
__device__ __forceinline__ float2 rotate(float2 v, float c0, float s0) {
  return make_float2(fmaf(v.x, c0, -__fmul_rn(v.y, s0)), fmaf(v.x, s0, __fmul_rn(v.y, c0)));
}

// The noise of one sample pair: one Philox call, two Box-Muller transforms, four N(0,1) (I, Q of the first sample, then the second)
__device__ __forceinline__ void noise4(uint32_t ctr, uint32_t flo, uint32_t site, uint32_t step, uint32_t k0, uint32_t k1,
                                       float* g) {
  const u32x4 z = philox4x32(ctr, flo, site, step, k0, k1);
  box_muller(z[0], z[1], g[0], g[1]);
  box_muller(z[2], z[3], g[2], g[3]);
}

// Workgroup scan of one value per thread, wrapping in T: -> the sum of the values of all threads below this one.  wsum: FR_WAVES
// words of LDS.  Holds a barrier: what every thread did before the call comes before what any thread does after it.
template <typename T>
__device__ __forceinline__ T scan_exclusive(T s, T* wsum, int lane, int wave) {
  T inc = s;
#pragma unroll
  for (int o = 1; o < IQ_WAVE; o <<= 1) {
    const T t = __shfl_up(inc, o, IQ_WAVE);
    if (lane >= o) inc += t;
  }
  if (lane == IQ_WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  T run = inc - s;
  for (int i = 0; i < wave; ++i) run += wsum[i];
  return run;
}

// The four wave sums of a workgroup in one fixed order
__device__ __forceinline__ float red_sum(const float* red) { return ((red[0] + red[1]) + red[2]) + red[3]; }

// The generators' tail, first half: the frame's mean power P from the per-thread sums pw (a barrier: the frame in LDS is complete
// behind it), rs = 1 / sqrt(P + 1e-12) and the noise sigma per component at snr_db.  red: FR_WAVES floats of LDS.
struct FrameScale {
  float P, rs, sig;
};
__device__ __forceinline__ FrameScale frame_scale(float pw, float* red, int len, int lane, int wave, bool noise, float snr_db) {
  pw = wave_sum(pw);
  if (lane == 0) red[wave] = pw;
  __syncthreads();
  FrameScale f;
  f.P = red_sum(red) / (float)len;
  f.rs = 1.f / sqrtf(f.P + 1e-12f);
  f.sig = noise ? sqrtf(0.5f * powf(10.f, -snr_db / 10.f)) : 0.f;
  return f;
}
// Second half: two consecutive samples per thread: normalise, add the noise of counter noise_ctr + pair, one 16-byte store (st4)
// or two 8-byte stores.  fr: the frame in LDS, (len + 1) / 2 pairs, the second half of an odd last pair zero.
__device__ __forceinline__ void store_frame(float* dst, const float2* fr, int len, int st4, int tid, FrameScale f, bool noise,
                                            uint32_t noise_ctr, uint32_t flo, uint32_t site, uint32_t step, uint32_t k0, uint32_t k1) {
  const int nq = (len + 1) >> 1;
  for (int p = tid; p < nq; p += FR_THREADS) {
    float4 v = reinterpret_cast<const float4*>(fr)[p];
    v.x *= f.rs; v.y *= f.rs; v.z *= f.rs; v.w *= f.rs;
    if (noise) {
      float g[4];
      noise4(noise_ctr + (uint32_t)p, flo, site, step, k0, k1, g);
      v.x = fmaf(f.sig, g[0], v.x); v.y = fmaf(f.sig, g[1], v.y);
      v.z = fmaf(f.sig, g[2], v.z); v.w = fmaf(f.sig, g[3], v.w);
    }
    if (st4) {
      reinterpret_cast<float4*>(dst)[p] = v;
    } else {
      reinterpret_cast<float2*>(dst)[2 * p] = make_float2(v.x, v.y);
      if (2 * p + 1 < len) reinterpret_cast<float2*>(dst)[2 * p + 1] = make_float2(v.z, v.w);
    }
  }
}

// ---- symbol stages (carrier.hip, equaliser.hip): sample n of a frame in either layout, planar [2][len] or interleaved [len][2]
__device__ __forceinline__ float2 load_sample(const float* fr, int len, int planar, int n) {
  return planar ? make_float2(fr[n], fr[len + n]) : reinterpret_cast<const float2*>(fr)[n];
}
__device__ __forceinline__ void store_sample(float* fr, int len, int planar, int n, float2 v) {
  if (planar) {
    fr[n] = v.x;
    fr[len + n] = v.y;
  } else {
    reinterpret_cast<float2*>(fr)[n] = v;
  }
}

// ---- channelizers: planar (2, len) frames against a (c, s) table on v_mfma_f32_32x32x2_f32
typedef __attribute__((ext_vector_type(16))) float f32x16;

// accumulator register r of lane half h holds tile row (r & 3) + 8 * (r >> 2) + 4 * h; the column is lane & 31
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// floats of LDS of the frame [2][len] (I plane, then Q plane), rounded up to 16 bytes
__host__ __device__ inline int frame_floats(int len) { return (2 * len + 3) & ~3; }

// The frame into LDS, as it lies in memory.
__device__ __forceinline__ void stage_frame(float* dst, const float* src, int len, int vec4, int tid) {
  if (vec4) {
    for (int q = tid; q < len / 2; q += FR_THREADS) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
  } else {
    for (int q = tid; q < 2 * len; q += FR_THREADS) dst[q] = src[q];
  }
}

// First sample of column t's window, clamped to [-n_fft, len]: with m in [0, n_fft) a clamped start gives an index outside
// [0, len) exactly when the true one is outside.
__device__ __forceinline__ int window_start(long t, int n_fft, int hop, int pad, int len) {
  long j = t * (long)hop - (long)pad;
  j = j < -(long)n_fft ? -(long)n_fft : j;
  return (int)(j > (long)len ? (long)len : j);
}

// One step of a 32-bin x 32-column tile: this lane's window sample j (0 outside [0, len): a select, never a read) against its
// table entries (ac, as).   Re += c*I + s*Q,   Im += c*Q - s*I
__device__ __forceinline__ void channel_step(f32x16& re, f32x16& im, float ac, float as, const float* fI, const float* fQ, int j,
                                             int len) {
  const bool in = (unsigned)j < (unsigned)len;
  const int jc = in ? j : 0;
  const float bi = in ? fI[jc] : 0.f, bq = in ? fQ[jc] : 0.f;
  re = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bi, re, 0, 0, 0);
  re = __builtin_amdgcn_mfma_f32_32x32x2f32(as, bq, re, 0, 0, 0);
  im = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bq, im, 0, 0, 0);
  im = __builtin_amdgcn_mfma_f32_32x32x2f32(-as, bi, im, 0, 0, 0);
}

// The last step of the channelizers' adjoints (spectrogram_bwd_kernel, cyclic_bwd_kernel): the overlap-add of one tile of
// per-column products.  g holds G[m][c] for the window samples m in [mlo, mhi) (mlo a multiple of 32) of the columns t0 + c,
// c < tcols, in segments of 32 samples: sample m at g + ((m - mlo) >> 5) * seg + (m & 31) * row + c; with PLANES = 2 the Q
// product lies `plane` floats behind the I product and goes to dxq.  Thread j % FR_THREADS adds to sample j the products of
// the columns whose window covers it, in ascending t: one owner per sample, no atomics, no dependence on timing.
template <int PLANES>
__device__ __forceinline__ void overlap_add(float* dxi, float* dxq, const float* g, int seg, int row, int plane, long t0,
                                            int tcols, long hop, long pad, long mlo, long mhi, int len, int tid) {
  long jlo = t0 * hop - pad + mlo, jhi = (t0 + tcols - 1) * hop - pad + mhi - 1;   // first and last sample touched
  jlo = jlo < 0 ? 0 : jlo;
  jhi = jhi > len - 1 ? len - 1 : jhi;
  for (long j = jlo + ((tid - jlo) & (FR_THREADS - 1)); j <= jhi; j += FR_THREADS) {
    float si = 0.f, sq = 0.f;
    for (int c = 0; c < tcols; ++c) {
      const long m = j + pad - (t0 + c) * hop;
      if (m >= mlo && m < mhi) {
        const float* e = g + (int)((m - mlo) >> 5) * seg + (int)(m & 31) * row + c;
        si += e[0];
        if (PLANES == 2) sq += e[plane];
      }
    }
    dxi[j] += si;
    if (PLANES == 2) dxq[j] += sq;
  }
}

// The image value of one (re, im): power, the level (mode 0: the power, mode 1: log10(P + floor)), then v * scale + shift.
// (cyclic.hip has a third level and keeps its own three-way choice between power and scale_shift.)
__device__ __forceinline__ float power(float re, float im, float inv_norm) { return fmaf(im, im, re * re) * inv_norm; }
__device__ __forceinline__ float scale_shift(float v, float scale, float shift) { return __fadd_rn(__fmul_rn(v, scale), shift); }
__device__ __forceinline__ float image_value(float re, float im, float inv_norm, int mode, float floor, float scale, float shift) {
  const float P = power(re, im, inv_norm);
  return scale_shift(mode ? log10f(P + floor) : P, scale, shift);
}
