// A fading channel on the device (iq_frames_fade, include/iqvit.h): up to 8 taps whose gains are sums of rotating paths (Clarke's
// model: a line of sight and up to 32 scatterers, each with its own Doppler shift), read at positions that drift with a
// sample-clock offset through a fractional-delay interpolator.  It takes any raw (n, len_in, 2) frames and gives (n, len_out, 2)
// frames; the tail (power, unit-power scaling, AWGN, store) is frame_scale + store_frame of frames.h, the generators' own.
//
// Time is an int64 in units of 2^-32 sample and phase an int32 in units of 2^-32 turn: there is no floating-point time or phase
// anywhere before the one conversion of e(p), so sample 8191 of a frame is as exact as sample 0.
//
// One workgroup per frame.  LDS: the output frame | the input frame | the interpolation table | the path table (phase, inc)
// [8][33] | the amplitudes [8][33] | the wave sums.
//   1. the input frame and the tables go to LDS; in IQ_FADE_DRAWN thread j < 264 draws slot j of the path table
//   2. sample n = 256 k + tid: per tap l the position Q, the K-point interpolation (an fmaf chain over LDS) and the gain
//      g_l[n], a sum over the paths s ascending of amp e(phase + n inc); y[n] = sum_l rot(r_l, g_l) into the output frame in LDS.
//      A thread works on FD_U = 2 of its samples at a time (n and n + 256): a batch of 256 frames is one wave per SIMD, and two
//      independent chains in the loop over the paths are what there is to overlap.  The bits are those of one sample at a time.
//   3. frame_scale + store_frame
// Lanes split SAMPLES, never paths: a lane owns its sample's whole sum, so the order of every sum is the loop order (no
// cross-lane reduction but the power's), every read of the path table is one address for the whole wave (an LDS broadcast, no
// bank conflict), `amp == 0` is a wave-uniform branch, and the K reads of neighbouring lanes are neighbouring float2 (the lanes of
// a wave read 64 consecutive samples, shifted by at most a few samples by the drift).
// Every LDS index is below its array's size by construction: the frame reads pass a range check whose failure selects 0
// (never a read), f < n_frac because the fraction is below 2^32, slots are l * 33 + s with l < 8, s <= 32.
//
// Random numbers (IQ_FADE_DRAWN, and the noise in both modes): the key of the generators (frames.h frame_key), counter =
// (c, frame lo, IQ_SITE_FADE, stream); c = 0xFFFFFFFF the frame's parameters, c = 0xFFFFF000 + l * 33 + s path s of tap l,
// c = 0x80000000 + p the noise of samples 2p and 2p + 1.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int FD_MAX_TAPS = 8, FD_MAX_SIN = 32, FD_PATHS = FD_MAX_SIN + 1, FD_MAX_K = 16, FD_MAX_FRAC = 256;
constexpr int FD_SLOTS = FD_MAX_TAPS * FD_PATHS;      // 264
constexpr uint32_t FD_PATH_CTR = 0xFFFFF000u;         // .. + 263: never a noise group (len * 8 <= 64 KB) or the parameters
constexpr uint32_t FD_NOISE_CTR = 0x80000000u;
constexpr size_t FD_LDS_BYTES = 160 * 1024;
constexpr int FD_U = 2;                              // samples a thread keeps in flight

struct FdArgs {
  const float* x;
  float* y;
  int32_t* paths_out;
  float* amps_out;
  int64_t* clock_out;
  const float* interp;
  const float* snr_db;
  const int32_t* paths;
  const float* amps;
  const int64_t* clock;
  int mode, len_in, len_out, n_taps, n_sin, K, n_frac, normalise, timing;
  int ld4, st4;         // every frame of x / y starts 16-byte aligned (len even): float4 loads / stores
  int32_t start, d_lo;
  uint32_t d_span;      // d_hi - d_lo + 1
  float fd_lo, fd_hi, sin_scale;
  uint64_t seed, frame_base;
  uint32_t stream;
  int32_t delay[FD_MAX_TAPS];
  float los[FD_MAX_TAPS], tap_sigma[FD_MAX_TAPS];
};

// v[i], i < 8, without a per-lane index into the kernel arguments
__device__ __forceinline__ float pick8(const float* v, int i) {
  float r = v[0];
#pragma unroll
  for (int k = 1; k < FD_MAX_TAPS; ++k) r = i == k ? v[k] : r;
  return r;
}

__host__ __device__ inline size_t fade_lds_bytes(int len_in, int len_out, int K, int n_frac) {
  return (size_t)((len_out + 1) / 2) * 16 + (size_t)((len_in + 1) / 2) * 16 + (size_t)((n_frac * K + 3) & ~3) * 4 +
         (size_t)FD_SLOTS * (sizeof(int2) + sizeof(float)) + FR_WAVES * sizeof(float);
}

__global__ __launch_bounds__(FR_THREADS) void frames_fade_kernel(FdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6;
  const long fi = blockIdx.x;
  const int len_in = a.len_in, len_out = a.len_out, K = a.K, nt = a.n_frac * K;
  float2* fo = reinterpret_cast<float2*>(lds);
  float2* fx = fo + 2 * ((len_out + 1) >> 1);
  float* tab = reinterpret_cast<float*>(fx + 2 * ((len_in + 1) >> 1));
  int2* pth = reinterpret_cast<int2*>(tab + ((nt + 3) & ~3));
  float* amp = reinterpret_cast<float*>(pth + FD_SLOTS);
  float* red = amp + FD_SLOTS;

  const FrameKey key = frame_key(a.seed, a.frame_base, blockIdx.x);
  const uint32_t k0 = key.k0, k1 = key.k1, flo = key.flo;

  // ---- the input frame and the interpolation table, as they lie in memory
  {
    const float* src = a.x + fi * len_in * 2;
    if (a.ld4) {
      for (int q = tid; q < len_in / 2; q += FR_THREADS) reinterpret_cast<float4*>(fx)[q] = reinterpret_cast<const float4*>(src)[q];
    } else {
      for (int q = tid; q < 2 * len_in; q += FR_THREADS) reinterpret_cast<float*>(fx)[q] = src[q];
    }
    for (int i = tid; i < nt; i += FR_THREADS) tab[i] = a.interp[i];
  }

  // ---- the clock and the path table: given, or drawn (every thread derives the same clock from the same four words)
  int64_t T0, S;
  if (a.mode == IQ_FADE_GIVEN) {
    for (int j = tid; j < FD_SLOTS; j += FR_THREADS) {
      pth[j] = reinterpret_cast<const int2*>(a.paths)[fi * FD_SLOTS + j];
      amp[j] = a.amps[fi * FD_SLOTS + j];
    }
    T0 = a.clock[2 * fi];
    S = a.clock[2 * fi + 1];
  } else {
    const u32x4 par = philox4x32(FR_PARAM_CTR, flo, IQ_SITE_FADE, a.stream, k0, k1);
    const int32_t d = (int32_t)((uint32_t)a.d_lo + __umulhi(par[0], a.d_span));
    T0 = (int64_t)(((uint64_t)(int64_t)a.start << 32) + (a.timing ? (uint64_t)par[1] : 0u));
    S = (int64_t)0x100000000ll + (int64_t)d;
    const float fd = fminf(fmaf(__fsub_rn(a.fd_hi, a.fd_lo), u24(par[2]), a.fd_lo), a.fd_hi);
    const double fd_inc = rint((double)fd * 4294967296.0);
    for (int j = tid; j < FD_SLOTS; j += FR_THREADS) {
      const int l = j / FD_PATHS, s = j - l * FD_PATHS;
      int2 pv = make_int2(0, 0);
      float av = 0.f;
      if (l < a.n_taps && s <= a.n_sin) {
        const u32x4 z = philox4x32(FD_PATH_CTR + (uint32_t)j, flo, IQ_SITE_FADE, a.stream, k0, k1);
        float sn, cs;
        sincospif(2.f * u24(z[1]), &sn, &cs);
        pv.x = s == 0 ? 0 : (int32_t)z[0];
        pv.y = (int32_t)(uint32_t)(uint64_t)(int64_t)rint(fd_inc * (double)cs);
        av = s == 0 ? pick8(a.los, l) : __fmul_rn(pick8(a.tap_sigma, l), a.sin_scale);
      }
      pth[j] = pv;
      amp[j] = av;
    }
  }
  __syncthreads();
  for (int j = tid; j < FD_SLOTS; j += FR_THREADS) {
    if (a.paths_out) reinterpret_cast<int2*>(a.paths_out)[fi * FD_SLOTS + j] = pth[j];
    if (a.amps_out) a.amps_out[fi * FD_SLOTS + j] = amp[j];
  }
  if (a.clock_out && tid == 0) {
    a.clock_out[2 * fi] = T0;
    a.clock_out[2 * fi + 1] = S;
  }

  // ---- y[n] = sum_l rot(r_l[n], g_l[n]) into fo, and its power
  const int c = (K - 1) >> 1, L = a.n_taps, ns = a.n_sin;
  const uint64_t nf = (uint64_t)a.n_frac;
  float pw = 0.f;
  for (int n0 = tid; n0 < len_out; n0 += FD_U * FR_THREADS) {
    // FD_U samples of this thread in flight (n0, n0 + 256, ..): independent chains for one wave per SIMD to overlap.  A sample
    // beyond len_out is computed like any other (its reads pass the same range check) and not stored.
    float yr[FD_U], yi[FD_U];
#pragma unroll
    for (int u = 0; u < FD_U; ++u) yr[u] = yi[u] = 0.f;
    for (int l = 0; l < L; ++l) {
      float rr[FD_U], ri[FD_U], gr[FD_U], gi[FD_U];
#pragma unroll
      for (int u = 0; u < FD_U; ++u) {
        const int64_t Q = T0 + (int64_t)(n0 + u * FR_THREADS) * S - ((int64_t)a.delay[l] << 16);
        const int64_t m = (Q >> 32) - c;
        const int f = (int)(((uint64_t)(uint32_t)Q * nf) >> 32);
        const float* row = tab + f * K;
        rr[u] = ri[u] = gr[u] = gi[u] = 0.f;
        for (int k = 0; k < K; ++k) {
          const int64_t idx = m + k;
          const bool in = (uint64_t)idx < (uint64_t)len_in;
          const float2 xv = fx[in ? (int)idx : 0];
          const float vr = in ? xv.x : 0.f, vi = in ? xv.y : 0.f, w = row[k];
          rr[u] = k == 0 ? __fmul_rn(vr, w) : fmaf(vr, w, rr[u]);
          ri[u] = k == 0 ? __fmul_rn(vi, w) : fmaf(vi, w, ri[u]);
        }
      }
      const int2* pl = pth + l * FD_PATHS;
      const float* al = amp + l * FD_PATHS;
      for (int s = 0; s <= ns; ++s) {
        const float av = al[s];
        if (av != 0.f) {
          const int2 pv = pl[s];
#pragma unroll
          for (int u = 0; u < FD_U; ++u) {
            const uint32_t p = (uint32_t)pv.x + (uint32_t)(n0 + u * FR_THREADS) * (uint32_t)pv.y;
            float sn, cs;
            sincospif((float)(int32_t)p * 0x1p-31f, &sn, &cs);
            gr[u] = fmaf(av, cs, gr[u]);
            gi[u] = fmaf(av, sn, gi[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < FD_U; ++u) {
        const float2 t = rotate(make_float2(rr[u], ri[u]), gr[u], gi[u]);
        yr[u] = __fadd_rn(yr[u], t.x);
        yi[u] = __fadd_rn(yi[u], t.y);
      }
    }
#pragma unroll
    for (int u = 0; u < FD_U; ++u) {
      const int n = n0 + u * FR_THREADS;
      if (n < len_out) {
        fo[n] = make_float2(yr[u], yi[u]);
        pw = fmaf(yi[u], yi[u], fmaf(yr[u], yr[u], pw));
      }
    }
  }
  if ((len_out & 1) && tid == 0) fo[len_out] = make_float2(0.f, 0.f);      // the second half of the last pair

  const float snr = a.snr_db ? a.snr_db[fi] : nanf("");
  const bool noise = snr == snr;
  FrameScale fs = frame_scale(pw, red, len_out, lane, wave, noise, snr);
  if (!a.normalise) fs.rs = 1.f;
  store_frame(a.y + fi * len_out * 2, fo, len_out, a.st4, tid, fs, noise, FD_NOISE_CTR, flo, IQ_SITE_FADE, a.stream, k0, k1);
}

inline bool nonneg_finite(float v) { return v >= 0.f && v < INFINITY; }

}  // namespace

extern "C" int iq_frames_fade(const float* x, float* y, int32_t* paths_out, float* amps_out, int64_t* clock_out, int n_frames,
                              int len_out, const iq_fading_t* par, iq_stream_t stream) {
  if (!x || !y || !par || !par->interp) return IQ_ERR_ARG;
  if (par->mode < IQ_FADE_GIVEN || par->mode > IQ_FADE_DRAWN) return IQ_ERR_ARG;
  if (par->mode == IQ_FADE_GIVEN && (!par->paths || !par->amps || !par->clock)) return IQ_ERR_ARG;
  if (len_out < 1 || par->len_in < 1) return IQ_ERR_ARG;
  if (par->n_taps < 1 || par->K < 1 || par->n_frac < 1 || par->n_sin < 0) return IQ_ERR_ARG;
  if ((par->normalise & ~1) || (par->timing & ~1)) return IQ_ERR_ARG;
  for (int l = 0; l < par->n_taps && l < FD_MAX_TAPS; ++l)
    if (par->delay[l] < 0 || !nonneg_finite(par->los[l]) || !nonneg_finite(par->tap_sigma[l])) return IQ_ERR_ARG;
  if (!nonneg_finite(par->fd_lo) || !nonneg_finite(par->fd_hi) || par->fd_hi > 0.5f || par->fd_lo > par->fd_hi) return IQ_ERR_ARG;
  if (par->d_lo > par->d_hi || (int64_t)par->d_hi - (int64_t)par->d_lo >= 0xFFFFFFFFll) return IQ_ERR_ARG;
  if (((uintptr_t)x & 7) || ((uintptr_t)y & 7) || ((uintptr_t)paths_out & 7) || ((uintptr_t)amps_out & 3) ||
      ((uintptr_t)clock_out & 7) || ((uintptr_t)par->interp & 3) || ((uintptr_t)par->snr_db & 3) || ((uintptr_t)par->paths & 7) ||
      ((uintptr_t)par->amps & 3) || ((uintptr_t)par->clock & 7))
    return IQ_ERR_ARG;
  if (par->n_taps > FD_MAX_TAPS || par->n_sin > FD_MAX_SIN || par->K > FD_MAX_K || par->n_frac > FD_MAX_FRAC) return IQ_ERR_UNSUPPORTED;
  if (!frame_fits(len_out) || !frame_fits(par->len_in)) return IQ_ERR_UNSUPPORTED;
  const size_t lds = fade_lds_bytes(par->len_in, len_out, par->K, par->n_frac);
  if (lds > FD_LDS_BYTES) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  FdArgs a;
  a.x = x; a.y = y; a.paths_out = paths_out; a.amps_out = amps_out; a.clock_out = clock_out;
  a.interp = par->interp; a.snr_db = par->snr_db; a.paths = par->paths; a.amps = par->amps; a.clock = par->clock;
  a.mode = par->mode; a.len_in = par->len_in; a.len_out = len_out; a.n_taps = par->n_taps; a.n_sin = par->n_sin;
  a.K = par->K; a.n_frac = par->n_frac; a.normalise = par->normalise; a.timing = par->timing;
  a.ld4 = frame_vec4(x, par->len_in);
  a.st4 = frame_vec4(y, len_out);
  a.start = par->start; a.d_lo = par->d_lo;
  a.d_span = (uint32_t)((int64_t)par->d_hi - (int64_t)par->d_lo + 1);
  a.fd_lo = par->fd_lo; a.fd_hi = par->fd_hi;
  a.sin_scale = par->n_sin > 0 ? sqrtf(2.f / (float)par->n_sin) : 0.f;
  a.seed = par->seed; a.frame_base = par->frame_base; a.stream = par->stream;
  for (int l = 0; l < FD_MAX_TAPS; ++l) {
    const bool in = l < par->n_taps;
    a.delay[l] = in ? par->delay[l] : 0;
    a.los[l] = in ? par->los[l] : 0.f;
    a.tap_sigma[l] = in ? par->tap_sigma[l] : 0.f;
  }
  const double evals = (double)n_frames * len_out * par->n_taps * (par->n_sin + 1);
  const double bytes = (double)n_frames * ((double)(par->len_in + len_out) * 8 + (paths_out ? FD_SLOTS * 8 : 0) + (amps_out ? FD_SLOTS * 4 : 0));
  IQ_PROF_K(bytes, evals * 4 + (double)n_frames * len_out * par->n_taps * (4.0 * par->K + 8), "frames_fade_kernel");
  launch_frames(frames_fade_kernel, n_frames, lds, st, a);
  return iq_launch_status();
}
