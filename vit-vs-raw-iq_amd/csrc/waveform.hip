// Pulse-shaped labelled I/Q frames made on the device (iq_frames_waveform, include/iqvit.h): the transmitter of synth.hip at
// `sps` samples per symbol -- a polyphase FIR over the symbols (any pulse: the tables are plain numbers, waveform.py fills them
// with a root-raised cosine), true OQPSK (the Q rail half a symbol late), CPM from an integer phase-increment table (GMSK), one
// timing phase per frame, and a static multipath channel of up to 8 taps (tap 0 Rician, the rest Rayleigh) between the shaping
// and the carrier phase.  The keying, the class / SNR draw, the rotation and the tail (unit power, AWGN, store) are the
// functions of frames.h that frames_synth_kernel calls: with sps = span = n_phase = 1, a pulse of 1.0 and one tap the frames
// are those of iq_frames_synth, bit for bit.
//
// One workgroup per frame, the frame in LDS.
//   1. symbol words -> integers in LDS (NS of them, 4 per Philox call) and, if asked for, to `symbols`; the frame's slice
//      [sps][span] of the pulse table, its class's constellation (up to WF_POINTS_LDS points) and its channel taps go to LDS too
//   2. u[n'], n' < len + L - 1: kinds 0 and 2 a product and span - 1 fmaf per component, strided over the workgroup; kind 1 a
//      wrapping int32 prefix sum of the phase increments (each thread owns a contiguous chunk and computes its increments twice,
//      once for the chunk sum and once for the running phase: no increment array), float only at the sincospi
//   3. v[n] = sum_l h_l u[n + L-1 - l] in rounds of 256 consecutive n: every thread reads its L inputs, the workgroup meets at a
//      barrier, every thread writes the rotated v[n] over u[n].  Round k writes [256 k, 256 k + 256) and reads up to
//      256 k + 255 + L - 1: no round reads what an earlier one wrote, and the barrier of round k + 1 comes after every read of
//      round k.  With L = 1 there is no barrier and nothing but the rotation.
//   4. power, normalisation, noise, one 16-byte store per two samples: frame_scale + store_frame
// Every LDS index is below NS (symbols: the largest is (len + L - 2 + sps/2) / sps + span - 1 <= NS - 1), below len + L - 1
// (frame) or below sps * span (table) by construction.
//
// Random numbers: the keying and the site of synth.hip (key = (seed lo, seed hi ^ frame hi), counter = (c, frame lo,
// IQ_SITE_SYNTH, stream)); c = 0xFFFFFFFF the frame's parameters (word 3: the timing phase), c = 0xFFFFFFF0 + t the channel taps
// 2t and 2t + 1, c = p < 0x80000000 symbol words 4p..4p+3, c = 0x80000000 + p the noise of samples 2p and 2p + 1.
#include <math.h>

#include "frames.h"
#include "iqvit.h"
#include "prof.h"

namespace {

constexpr int WF_MAX_SPS = 16, WF_MAX_SPAN = 32, WF_MAX_PHASE = 64, WF_MAX_TAPS = 8;
constexpr int WF_POINTS_LDS = 1024;               // a constellation up to this size is read from LDS, a larger one from memory
constexpr uint32_t WF_TAP_CTR = 0xFFFFFFF0u;      // .. 0xFFFFFFF3: never a symbol or noise group (len * 8 <= 64 KB)
constexpr uint32_t WF_NOISE_CTR = 0x80000000u;

struct WfArgs {
  float* raw;
  int64_t* labels;
  float* snr;
  float* drawn;
  int32_t* symbols;
  float* taps;
  const float2* points;
  const float* pulse;
  const int32_t* fpulse;
  int len, n_classes, n_snrs, balanced;
  int sps, span, n_phase, timing, n_taps;
  int ns;       // symbol words of a frame: (len + L - 1 + sps) / sps + span
  int npts;     // float2 slots of LDS for the constellation
  uint64_t seed, frame_base;
  uint32_t stream;
  int st4;      // every frame of raw starts 16-byte aligned (len even): float4 stores
  float los;
  float tap_sigma[WF_MAX_TAPS];
  iq_synth_class_t classes[IQ_SYNTH_MAX_CLASSES];
  float snrs_db[IQ_SYNTH_MAX_SNRS];
};
static_assert(sizeof(WfArgs) <= 4096, "kernel arguments");

template <bool NOISE>
__global__ __launch_bounds__(FR_THREADS) void frames_waveform_kernel(WfArgs a) {
  // [nq][4] the frame (I,Q interleaved), len + L - 1 samples | [nw][4] the symbols as integers | [sps][span] the table slice |
  // the constellation | 8 taps | wave sums
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & (IQ_WAVE - 1), wave = tid >> 6, len = a.len;
  const long fi = blockIdx.x;
  const int L = a.n_taps, sps = a.sps, span = a.span, ns = a.ns;
  const int nu = len + L - 1;             // shaped samples
  const int nw = (ns + 3) >> 2;           // Philox calls of the symbol stream
  const int nt = sps * span;
  float2* fr = reinterpret_cast<float2*>(lds);
  int* w = reinterpret_cast<int*>(lds + 4 * ((nu + 1) >> 1));
  float* tab = reinterpret_cast<float*>(w + 4 * nw);
  float2* pts = reinterpret_cast<float2*>(tab + ((nt + 3) & ~3));
  float2* h = pts + a.npts;
  float* red = reinterpret_cast<float*>(h + WF_MAX_TAPS);
  uint32_t* wsum = reinterpret_cast<uint32_t*>(red + FR_WAVES);

  // ---- the frame's parameters: every thread derives the same values from the same four words
  const FrameKey key = frame_key(a.seed, a.frame_base, blockIdx.x);
  const uint32_t k0 = key.k0, k1 = key.k1, flo = key.flo;
  const u32x4 par = philox4x32(FR_PARAM_CTR, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
  const float turn = u24(par[0]);
  int cls, si;
  draw_class_snr(key.frame, par, a.balanced, a.n_classes, a.n_snrs, NOISE, cls, si);
  const int q = a.timing ? (int)__umulhi(par[3], (uint32_t)a.n_phase) : 0;
  const iq_synth_class_t cd = a.classes[cls];
  const int kind = cd.kind;               // frame-uniform: no branch below diverges
  const bool staged = kind == 0 && cd.count <= a.npts;
  float c0, s0;
  sincospif(2.f * turn, &s0, &c0);

  // ---- symbol words -> integers in LDS: the constellation index, the bit, 2 I + Q
  for (int p = tid; p < nw; p += FR_THREADS) {
    const u32x4 z = philox4x32((uint32_t)p, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
    int4 v;
    if (kind == 0) {
      v = make_int4((int)__umulhi(z[0], (uint32_t)cd.count), (int)__umulhi(z[1], (uint32_t)cd.count),
                    (int)__umulhi(z[2], (uint32_t)cd.count), (int)__umulhi(z[3], (uint32_t)cd.count));
    } else if (kind == 1) {
      v = make_int4((int)(z[0] & 1u), (int)(z[1] & 1u), (int)(z[2] & 1u), (int)(z[3] & 1u));
    } else {
      v = make_int4((int)(2u * (z[0] & 1u) + ((z[0] >> 1) & 1u)), (int)(2u * (z[1] & 1u) + ((z[1] >> 1) & 1u)),
                    (int)(2u * (z[2] & 1u) + ((z[2] >> 1) & 1u)), (int)(2u * (z[3] & 1u) + ((z[3] >> 1) & 1u)));
    }
    reinterpret_cast<int4*>(w)[p] = v;
    if (a.symbols) {
      int32_t* dst = a.symbols + fi * ns;
      const int k = 4 * p;
      if (k < ns) dst[k] = v.x;
      if (k + 1 < ns) dst[k + 1] = v.y;
      if (k + 2 < ns) dst[k + 2] = v.z;
      if (k + 3 < ns) dst[k + 3] = v.w;
    }
  }
  // the table slice of timing phase q, as the 32-bit words it is made of (fp32 for kinds 0 and 2, int32 for kind 1)
  {
    const uint32_t* src = kind == 1 ? reinterpret_cast<const uint32_t*>(a.fpulse) : reinterpret_cast<const uint32_t*>(a.pulse);
    src += (size_t)q * nt;
    for (int i = tid; i < nt; i += FR_THREADS) reinterpret_cast<uint32_t*>(tab)[i] = src[i];
  }
  if (staged)
    for (int i = tid; i < cd.count; i += FR_THREADS) pts[i] = a.points[cd.offset + i];
  // the channel: tap l from words (0,1) (l even) or (2,3) (l odd) of counter 0xFFFFFFF0 + l/2; one tap (1, 0) without it
  if (tid < WF_MAX_TAPS) {
    float2 hv = make_float2(0.f, 0.f);
    if (L == 1) {
      if (tid == 0) hv = make_float2(1.f, 0.f);
    } else if (tid < L) {
      const u32x4 z = philox4x32(WF_TAP_CTR + (uint32_t)(tid >> 1), flo, IQ_SITE_SYNTH, a.stream, k0, k1);
      float g0, g1;
      if (tid & 1) box_muller(z[2], z[3], g0, g1);
      else box_muller(z[0], z[1], g0, g1);
      const float sg = a.tap_sigma[tid];
      hv = make_float2((tid == 0 ? a.los : 0.f) + sg * g0, sg * g1);
    }
    h[tid] = hv;
    if (a.taps) reinterpret_cast<float2*>(a.taps)[fi * WF_MAX_TAPS + tid] = hv;
  }
  __syncthreads();

  // ---- the shaped signal u[n'], n' < nu, into fr
  if (kind == 1) {
    // CPM: PHI[n'] = sum_{j <= n'} inc[j] mod 2^32, inc[j] = sum_i b[j/sps + i] * fpulse[q][j%sps][i].  Thread t owns [start, end).
    const uint32_t* ft = reinterpret_cast<const uint32_t*>(tab);
    const int chunk = (nu + FR_THREADS - 1) / FR_THREADS;
    const int start = min(tid * chunk, nu), end = min(start + chunk, nu);
    auto inc_at = [&](int m, int r) {
      uint32_t s = 0;
      for (int i = 0; i < span; ++i) s += (uint32_t)(2 * w[m + i] - 1) * ft[r * span + i];
      return s;
    };
    uint32_t s = 0;
    int m = start / sps, r = start - m * sps;
    for (int n = start; n < end; ++n) {
      s += inc_at(m, r);
      if (++r == sps) { r = 0; ++m; }
    }
    uint32_t run = scan_exclusive(s, wsum, lane, wave);
    m = start / sps; r = start - m * sps;
    for (int n = start; n < end; ++n) {
      run += inc_at(m, r);
      if (++r == sps) { r = 0; ++m; }
      float sn, cs;
      sincospif((float)(int32_t)run * 0x1p-31f, &sn, &cs);
      fr[n] = make_float2(cs, sn);
    }
  } else if (kind == 0) {
    const float2* gp = a.points + cd.offset;
    for (int n = tid; n < nu; n += FR_THREADS) {
      const int m = n / sps, r = n - m * sps;
      const float* pr = tab + r * span;
      const float2 a0 = staged ? pts[w[m]] : gp[w[m]];
      float ur = a0.x * pr[0], ui = a0.y * pr[0];
      for (int i = 1; i < span; ++i) {
        const float2 ai = staged ? pts[w[m + i]] : gp[w[m + i]];
        ur = fmaf(ai.x, pr[i], ur);
        ui = fmaf(ai.y, pr[i], ui);
      }
      fr[n] = make_float2(ur, ui);
    }
  } else {
    // OQPSK: the I rail at n', the Q rail at n' + sps/2
    const int half = sps >> 1;
    for (int n = tid; n < nu; n += FR_THREADS) {
      const int m = n / sps, r = n - m * sps;
      const int m2 = (n + half) / sps, r2 = n + half - m2 * sps;
      const float* pr = tab + r * span;
      const float* pr2 = tab + r2 * span;
      float ur = ((w[m] & 2) ? FR_RSQRT2 : -FR_RSQRT2) * pr[0];
      float ui = ((w[m2] & 1) ? FR_RSQRT2 : -FR_RSQRT2) * pr2[0];
      for (int i = 1; i < span; ++i) {
        ur = fmaf((w[m + i] & 2) ? FR_RSQRT2 : -FR_RSQRT2, pr[i], ur);
        ui = fmaf((w[m2 + i] & 1) ? FR_RSQRT2 : -FR_RSQRT2, pr2[i], ui);
      }
      fr[n] = make_float2(ur, ui);
    }
  }
  __syncthreads();

  // ---- channel, carrier phase, power.  Round k: n = 256 k + tid.
  float pw = 0.f, hp = 0.f;
  for (int l = 0; l < L; ++l) hp = fmaf(h[l].y, h[l].y, fmaf(h[l].x, h[l].x, hp));
  for (int base = 0; base < len; base += FR_THREADS) {
    const int n = base + tid;
    float2 v = make_float2(0.f, 0.f);
    if (n < len) {
      if (L > 1) {
        for (int l = 0; l < L; ++l) {
          const float2 hl = h[l], ul = fr[n + L - 1 - l];
          v.x += hl.x * ul.x - hl.y * ul.y;
          v.y += hl.x * ul.y + hl.y * ul.x;
        }
      } else {
        v = fr[n];
      }
    }
    if (L > 1) __syncthreads();
    if (n < len) {
      const float2 r = rotate(v, c0, s0);
      fr[n] = r;
      pw = fmaf(r.y, r.y, fmaf(r.x, r.x, pw));
    }
  }
  if (L == 1 && (len & 1) && tid == 0) fr[len] = make_float2(0.f, 0.f);     // the second half of the last pair
  const float snr = NOISE ? a.snrs_db[si] : nanf("");
  const FrameScale f = frame_scale(pw, red, len, lane, wave, NOISE, snr);
  if (tid == 0) {
    a.labels[fi] = cls;
    a.snr[fi] = snr;
    if (a.drawn) {
      reinterpret_cast<float4*>(a.drawn)[2 * fi] = make_float4((float)cls, snr, FR_TWO_PI * turn, f.P);
      reinterpret_cast<float4*>(a.drawn)[2 * fi + 1] = make_float4((float)q, hp, 0.f, 0.f);
    }
  }
  store_frame(a.raw + fi * len * 2, fr, len, a.st4, tid, f, NOISE, WF_NOISE_CTR, flo, IQ_SITE_SYNTH, a.stream, k0, k1);
}

}  // namespace

extern "C" int iq_frames_waveform(float* raw, int64_t* labels, float* snr, float* drawn, int32_t* symbols, float* taps,
                                  int n_frames, int len, const iq_waveform_t* par, iq_stream_t stream) {
  if (!raw || !labels || !snr || !par) return IQ_ERR_ARG;
  if (len <= 0) return IQ_ERR_ARG;
  if (!synth_lists_ok(par->classes, par->n_classes, par->snrs_db, par->n_snrs, par->points, par->balanced)) return IQ_ERR_ARG;
  if (par->timing & ~1) return IQ_ERR_ARG;
  if (par->sps < 1 || par->span < 1 || par->n_phase < 1 || par->n_taps < 1) return IQ_ERR_ARG;
  if (((uintptr_t)raw & 7) || ((uintptr_t)labels & 7) || ((uintptr_t)snr & 3) || ((uintptr_t)drawn & 15) ||
      ((uintptr_t)symbols & 3) || ((uintptr_t)taps & 7) || ((uintptr_t)par->points & 7) || ((uintptr_t)par->pulse & 3) ||
      ((uintptr_t)par->fpulse & 3))
    return IQ_ERR_ARG;
  const int nc = par->n_classes < IQ_SYNTH_MAX_CLASSES ? par->n_classes : IQ_SYNTH_MAX_CLASSES;
  int npts = 0;
  for (int i = 0; i < nc; ++i) {
    const iq_synth_class_t& c = par->classes[i];
    if (c.kind == 1 ? !par->fpulse : !par->pulse) return IQ_ERR_ARG;
    if (c.kind == 0 && c.count <= WF_POINTS_LDS && c.count > npts) npts = c.count;
  }
  if (!is_finite(par->los)) return IQ_ERR_ARG;
  for (int l = 0; l < par->n_taps && l < WF_MAX_TAPS; ++l)
    if (!(par->tap_sigma[l] >= 0.f && par->tap_sigma[l] < INFINITY)) return IQ_ERR_ARG;
  if (par->sps > WF_MAX_SPS || par->span > WF_MAX_SPAN || par->n_phase > WF_MAX_PHASE || par->n_taps > WF_MAX_TAPS)
    return IQ_ERR_UNSUPPORTED;
  if (!frame_fits(len)) return IQ_ERR_UNSUPPORTED;
  if (par->n_classes > IQ_SYNTH_MAX_CLASSES || par->n_snrs > IQ_SYNTH_MAX_SNRS) return IQ_ERR_UNSUPPORTED;
  if (n_frames <= 0) return IQ_OK;
  hipStream_t st = (hipStream_t)stream;
  IQ_PROF(IQ_FAM_MISC, st);
  WfArgs a;
  a.raw = raw; a.labels = labels; a.snr = snr; a.drawn = drawn; a.symbols = symbols; a.taps = taps;
  a.points = reinterpret_cast<const float2*>(par->points);
  a.pulse = par->pulse; a.fpulse = par->fpulse;
  a.len = len; a.n_classes = par->n_classes; a.n_snrs = par->n_snrs; a.balanced = par->balanced;
  a.sps = par->sps; a.span = par->span; a.n_phase = par->n_phase; a.timing = par->timing; a.n_taps = par->n_taps;
  const int nu = len + par->n_taps - 1;
  a.ns = (nu + par->sps) / par->sps + par->span;
  a.npts = (npts + 1) & ~1;                     // the taps behind it stay 16-byte aligned
  a.seed = par->seed; a.frame_base = par->frame_base; a.stream = par->stream;
  a.st4 = frame_vec4(raw, len);
  a.los = par->los;
  for (int l = 0; l < WF_MAX_TAPS; ++l) a.tap_sigma[l] = l < par->n_taps ? par->tap_sigma[l] : 0.f;
  pack_synth_lists(a.classes, a.snrs_db, par->classes, par->n_classes, par->snrs_db, par->n_snrs);
  const bool noise = par->n_snrs > 0;
  const int nt = par->sps * par->span;
  const size_t lds = (size_t)((nu + 1) / 2) * 16 + (size_t)((a.ns + 3) / 4) * 16 + (size_t)((nt + 3) & ~3) * 4 +
                     (size_t)a.npts * sizeof(float2) + WF_MAX_TAPS * sizeof(float2) + FR_WAVES * (sizeof(float) + sizeof(uint32_t));
  const double bytes = (double)n_frames * ((double)len * 8 + 12 + (drawn ? 32 : 0) + (symbols ? (double)a.ns * 4 : 0) + (taps ? 64 : 0));
  IQ_PROF_K(bytes, 0.0, "frames_waveform_kernel<%s>", noise ? "true" : "false");
  launch_frames(noise ? frames_waveform_kernel<true> : frames_waveform_kernel<false>, n_frames, lds, st, a);
  return iq_launch_status();
}
