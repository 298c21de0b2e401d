// Channel impairments on the device (iq_frames_impair, include/iqvit.h): circular time shift, conjugation, carrier phase /
// quarter-turn / frequency-offset rotation, gain and complex AWGN applied to raw (len, 2) I/Q frames in front of the z-score
// and re-layout of iq_frames_preprocess (misc.hip).  Training augmentation (Huang et al. 2019: rotation, flip, Gaussian noise)
// and the physical axes of an accuracy curve (impairments.py).
//
// One workgroup per frame.  The frame is read from HBM once (16-byte loads) into LDS, its power is reduced across the
// workgroup while it is staged, and every thread then builds two consecutive OUTPUT samples: the shift is only an LDS index, so
// no global access is ever misaligned, and the two planar channels leave as 8-byte stores, 512 contiguous bytes per wave.
// Memory bound: len*8 bytes in, 2*take*4 bytes out (+ 32 bytes of `drawn`) per frame; the Philox rounds, Box-Muller and the
// sincos of a frequency offset are VALU work under that traffic.
//
// Random numbers: philox4x32 of common.h.  key = (seed lo, seed hi ^ frame hi), counter = (c, frame lo, IQ_SITE_IMPAIR, step)
// with frame = frame_base + blockIdx.x (frame_key of frames.h).  c = 0xFFFFFFFF gives the four words the frame's parameters
// are cut from; c = p gives the noise of output samples 2p and 2p+1 (noise4).  Nothing depends on the grid.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr float IMP_INV_TWO_PI = 0.15915494309189533577f;

struct ImpArgs {
  const float* raw;
  float* out;
  float* drawn;
  int len, take;
  float i_mean, i_std, q_mean, q_std;
  iq_impair_t imp;
  int vec4;   // every frame of raw starts 16-byte aligned (len even): float4 staging loads
  int st2;    // both channels of every output frame start 8-byte aligned (take even): float2 stores
};

__device__ __forceinline__ float draw(float lo, float hi, float u) { return fminf(fmaxf(fmaf(hi - lo, u, lo), lo), hi); }

template <bool NOISE>
__global__ __launch_bounds__(FR_THREADS) void frames_impair_kernel(ImpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [ceil(len/2)][4] the frame (I,Q interleaved), then FR_WAVES sums
  const int tid = threadIdx.x, len = a.len, take = a.take;
  const long fi = blockIdx.x;
  const int nq = (len + 1) >> 1;
  float* red = lds + 4 * nq;

  // ---- stage the frame, summing |s|^2 in one fixed order whichever load width is used
  const float* src = a.raw + fi * len * 2;
  float pw = 0.f;
  for (int q = tid; q < nq; q += FR_THREADS) {
    float4 v;
    if (a.vec4) {
      v = reinterpret_cast<const float4*>(src)[q];
    } else {
      const float2 lo = reinterpret_cast<const float2*>(src)[2 * q];
      const float2 hi = 2 * q + 1 < len ? reinterpret_cast<const float2*>(src)[2 * q + 1] : make_float2(0.f, 0.f);
      v = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
    reinterpret_cast<float4*>(lds)[q] = v;
    if (NOISE) pw = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, pw))));
  }
  if (NOISE) {
    pw = wave_sum(pw);
    if ((tid & (IQ_WAVE - 1)) == 0) red[tid >> 6] = pw;
  }

  // ---- the frame's parameters: every thread derives the same values from the same four words (under the loads' latency)
  const iq_impair_t& im = a.imp;
  const FrameKey key = frame_key(im.seed, im.frame_base, blockIdx.x);
  const uint32_t k0 = key.k0, k1 = key.k1, flo = key.flo;
  const u32x4 w = philox4x32(FR_PARAM_CTR, flo, IQ_SITE_IMPAIR, im.step, k0, k1);
  const float theta = draw(im.phase_lo, im.phase_hi, u24(w[0]));
  const float f = draw(im.cfo_lo, im.cfo_hi, u24(w[1]));
  const int k = im.rot90 ? (int)(w[2] & 3u) : 0;
  const int cj = im.conj ? (int)((w[2] >> 2) & 1u) : 0;
  const int s = (int)(((uint64_t)(w[2] >> 8) * (uint64_t)(im.shift_max + 1)) >> 24);
  const float g = powf(10.f, draw(im.gain_db_lo, im.gain_db_hi, (float)(w[3] >> 16) * 0x1p-16f) / 20.f);
  // phase in TURNS, reduced to [0,1) before the sincos: theta/2pi + k/4 + f*n
  const float turn0 = fmaf(theta, IMP_INV_TWO_PI, 0.25f * (float)k);
  const bool rot_id = turn0 == 0.f && f == 0.f;   // no rotation: pass the sample through (x*1 - y*0 would turn -0 into +0)
  float c0, s0;
  sincospif(2.f * (turn0 - floorf(turn0)), &s0, &c0);

  __syncthreads();

  float snr = nanf(""), sig = 0.f;
  if (NOISE) {
    snr = draw(im.snr_db_lo, im.snr_db_hi, (float)(w[3] & 0xFFFFu) * 0x1p-16f);
    const float P = (g * g) * (red_sum(red) / (float)len);
    sig = sqrtf(0.5f * P / powf(10.f, snr / 10.f));
  }
  if (tid == 0 && a.drawn) {
    float* d = a.drawn + fi * 8;
    d[0] = theta; d[1] = f; d[2] = (float)k; d[3] = (float)cj; d[4] = (float)s; d[5] = g; d[6] = snr; d[7] = sig;
  }

  // ---- two consecutive output samples per thread
  const float2* fr = reinterpret_cast<const float2*>(lds);
  float* oi = a.out + fi * 2 * take;
  float* oq = oi + take;
  const int npair = (take + 1) >> 1;
  for (int p = tid; p < npair; p += FR_THREADS) {
    float gn[4] = {0.f, 0.f, 0.f, 0.f};
    if (NOISE) noise4((uint32_t)p, flo, IQ_SITE_IMPAIR, im.step, k0, k1, gn);
    float ri[2], rq[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = 2 * p + j;
      int idx = n + s;                        // n <= len, s < len
      if (idx >= len) idx -= len;
      const float2 v = fr[idx];
      const float x = v.x, y = cj ? -v.y : v.y;
      float cs = c0, sn = s0;
      if (f != 0.f) {                         // frame-uniform branch
        float t = fmaf(f, (float)n, turn0);
        t -= floorf(t);
        sincospif(2.f * t, &sn, &cs);
      }
      const float xr = rot_id ? x : x * cs - y * sn;
      const float yr = rot_id ? y : x * sn + y * cs;
      float vi = g * xr, vq = g * yr;
      if (NOISE) {
        vi = fmaf(sig, gn[2 * j], vi);
        vq = fmaf(sig, gn[2 * j + 1], vq);
      }
      ri[j] = (vi - a.i_mean) / a.i_std;      // IEEE subtract and divide, as frames_preprocess_kernel
      rq[j] = (vq - a.q_mean) / a.q_std;
    }
    if (a.st2) {
      reinterpret_cast<float2*>(oi)[p] = make_float2(ri[0], ri[1]);
      reinterpret_cast<float2*>(oq)[p] = make_float2(rq[0], rq[1]);
    } else {
      oi[2 * p] = ri[0];
      oq[2 * p] = rq[0];
      if (2 * p + 1 < take) {
        oi[2 * p + 1] = ri[1];
        oq[2 * p + 1] = rq[1];
      }
    }
  }
}

bool range_ok(float lo, float hi) { return lo <= hi && is_finite(lo) && is_finite(hi) && hi - lo < INFINITY; }

}  // namespace

extern "C" int iq_frames_impair(const float* raw, float* out, float* drawn, int n_frames, int len, int take, const float* stats,
                                const iq_impair_t* imp, iq_stream_t stream) {
  if (!raw || !out || !stats || !imp) return IQ_ERR_ARG;
  if (len <= 0 || take <= 0 || take > len) return IQ_ERR_ARG;
  if (!(stats[1] > 0.f) || !(stats[3] > 0.f)) return IQ_ERR_ARG;
  if (((uintptr_t)raw & 7) || ((uintptr_t)out & 3) || ((uintptr_t)drawn & 3)) return IQ_ERR_ARG;
  if (!range_ok(imp->phase_lo, imp->phase_hi) || !range_ok(imp->cfo_lo, imp->cfo_hi) ||
      !range_ok(imp->gain_db_lo, imp->gain_db_hi))
    return IQ_ERR_ARG;
  const bool noise = !(imp->snr_db_lo != imp->snr_db_lo && imp->snr_db_hi != imp->snr_db_hi);   // both NaN: no noise
  if (noise && !range_ok(imp->snr_db_lo, imp->snr_db_hi)) return IQ_ERR_ARG;
  if ((imp->rot90 | imp->conj) & ~1) return IQ_ERR_ARG;
  if (imp->shift_max < 0 || imp->shift_max >= len) return IQ_ERR_ARG;
  if (!frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  ImpArgs a;
  a.raw = raw; a.out = out; a.drawn = drawn; a.len = len; a.take = take;
  a.i_mean = stats[0]; a.i_std = stats[1]; a.q_mean = stats[2]; a.q_std = stats[3];
  a.imp = *imp;
  a.vec4 = frame_vec4(raw, len);
  a.st2 = (take % 2 == 0 && ((uintptr_t)out & 7) == 0) ? 1 : 0;
  const size_t lds = (size_t)((len + 1) / 2) * 16 + FR_WAVES * sizeof(float);
  const double bytes = (double)n_frames * ((double)len * 8 + 2.0 * take * 4 + (drawn ? 32 : 0));
  IQ_PROF_K(bytes, 0.0, "frames_impair_kernel<%s>", noise ? "true" : "false");
  launch_frames(noise ? frames_impair_kernel<true> : frames_impair_kernel<false>, n_frames, lds, st, a);
  return iq_launch_status();
}
